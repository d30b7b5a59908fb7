"""The fine-grained (grounding) model end to end on the MI355X kernels: fused backbone -> FPN neck -> VLDyHead.

Mirrors fine_grained/maskrcnn_benchmark/modeling/detector/generalized_vl_rcnn.py:64-404 (GeneralizedVLRCNN) in the configuration every FIBER
yaml uses: SWINT.VERSION "fusion" with BACKBONE.FUSION_VERSION "v2" (fusion_in_backbone), RPN_ONLY, RPN_ARCHITECTURE "VLDYHEAD".  Same
submodule names, hence the checkpoint key prefixes `fusion_backbone.backbone.body.*` (fusion_swin.py), `fusion_backbone.backbone.fpn.*`
(fpn.py), `fusion_backbone.language_backbone.body.model.*` and `rpn.head.*` (grounding_inference.VLDyHeadModule): a reference grounding
checkpoint loads with load_state_dict.  train() reproduces the freezing rules that apply here (:163-240).

Differences in the call surface, none in the computation:
  * no tokenizer files are assumed: `captions` are tokenised only by a tokenizer the caller supplied (anything with the
    batch_encode_plus of :268-275); otherwise the caller passes tokenizer_input = {"input_ids", "attention_mask"};
  * training targets are grounding_train.GroundingTargets (fixed-shape device tensors carrying their positive map), the result the
    four-entry loss dict; eval returns grounding_inference.Detections instead of a list of BoxLists;
  * `images` is a padded [B, 3, H, W] tensor, a (tensor, image_sizes) pair, or an object with .tensors / .image_sizes (ImageList).
"""
import torch
import torch.nn as nn

from .. import ops
from . import roberta as RB
from .fpn import build_swint_fpn
from .fusion_swin import FusionSwinTransformer
from .grounding_inference import Detections, PackedPositiveMaps, VLDyHeadModule


def _need(cond, name, why):
    if not cond:
        raise NotImplementedError(f"{name}: {why}")


class GeneralizedVLRCNN(nn.Module):
    def __init__(self, cfg, tokenizer=None):
        super().__init__()
        m = cfg.MODEL
        fc = m.DYHEAD.FUSE_CONFIG
        _need(m.SWINT.VERSION == "fusion", "MODEL.SWINT.VERSION", "only \"fusion\" (fusion in the backbone) is built, as every FIBER yaml sets")
        _need(m.BACKBONE.FUSION_VERSION == "v2", "MODEL.BACKBONE.FUSION_VERSION", "only \"v2\" (fusion_swin_transformer_v2 / roberta_fused_model_v2) is built")
        _need(m.RPN_ONLY, "MODEL.RPN_ONLY", "the ROI heads are not built (every FIBER yaml is RPN-only)")
        _need(m.RPN_ARCHITECTURE == "VLDYHEAD", "MODEL.RPN_ARCHITECTURE", "only \"VLDYHEAD\" is built")
        _need(getattr(m.BACKBONE, "CONV_BODY", "SWINT-FPN-RETINANET") == "SWINT-FPN-RETINANET", "MODEL.BACKBONE.CONV_BODY",
              "only the SWINT-FPN-RETINANET wiring (stage 2 skipped, P6 / P7 on top) is built")
        _need(not fc.MLM_LOSS, "MODEL.DYHEAD.FUSE_CONFIG.MLM_LOSS", "the masked-language-modelling branch (random_word, :276-285) is out of scope")
        _need(not getattr(fc, "ADD_LINEAR_LAYER", False), "MODEL.DYHEAD.FUSE_CONFIG.ADD_LINEAR_LAYER", "the prompt-tuning linear layer is not built")
        _need(not getattr(m.RPN, "FORCE_BOXES", False), "MODEL.RPN.FORCE_BOXES", "proposals forced from the targets feed ROI heads, which are not built")
        _need(not getattr(m, "LINEAR_PROB", False), "MODEL.LINEAR_PROB", "linear probing is not built")
        _need(not getattr(m.RPN, "RETURN_FUSED_FEATURES", False), "MODEL.RPN.RETURN_FUSED_FEATURES", "fused features feed ROI heads, which are not built")
        _need(not getattr(m.LANGUAGE_BACKBONE, "MASK_SPECIAL", False) and not getattr(getattr(cfg, "DATASETS", None), "ONE_HOT", False),
              "LANGUAGE_BACKBONE.MASK_SPECIAL / DATASETS.ONE_HOT", "these rewrite the text mask on the non-fusion path only (:299-309)")
        self.cfg = cfg
        self.fusion_in_backbone = True
        self.tokenizer = tokenizer
        s = m.SWINT
        self.fusion_backbone = FusionSwinTransformer(embed_dim=s.EMBED_DIM, depths=tuple(s.DEPTHS), num_heads=tuple(s.NUM_HEADS),
                                                     window_size=s.WINDOW_SIZE, drop_path_rate=s.DROP_PATH_RATE, fpn=build_swint_fpn(cfg),
                                                     text_config=RB.roberta_base_config())
        self.rpn = VLDyHeadModule(cfg)
        self.roi_heads = None
        self.freeze_backbone = m.BACKBONE.FREEZE
        self.freeze_fpn = m.FPN.FREEZE
        self.freeze_rpn = m.RPN.FREEZE
        self.freeze_language_backbone = m.LANGUAGE_BACKBONE.FREEZE
        self.freeze_cls_logits = fc.USE_DOT_PRODUCT_TOKEN_LOSS
        if self.freeze_cls_logits:                                   # :141-145
            for p in self.rpn.head.cls_logits.parameters():
                p.requires_grad = False
        if self.freeze_language_backbone:                            # :147-151
            for p in self.fusion_backbone.language_backbone.parameters():
                p.requires_grad = False

    def train(self, mode=True):
        """Training mode with the frozen parts kept in eval (:163-240)."""
        super().train(mode)
        frozen = []
        if self.freeze_backbone:
            frozen.append(self.fusion_backbone.backbone.body)
        if self.freeze_fpn:
            frozen.append(self.fusion_backbone.backbone.fpn)
        if self.freeze_cls_logits:
            frozen.append(self.rpn.head.cls_logits)
        if self.freeze_language_backbone:
            frozen.append(self.fusion_backbone.language_backbone)
        for mod in frozen:
            mod.eval()
            for p in mod.parameters():
                p.requires_grad = False
        if self.freeze_rpn:                                          # :184-188: the head in eval, every rpn parameter frozen
            self.rpn.head.eval()
            for p in self.rpn.parameters():
                p.requires_grad = False
        return self

    def _tokenize(self, captions, device):
        if self.tokenizer is None:
            raise ValueError("GeneralizedVLRCNN: captions need a tokenizer (pass tokenizer= to the constructor), or pass tokenizer_input")
        lb = self.cfg.MODEL.LANGUAGE_BACKBONE
        tok = self.tokenizer.batch_encode_plus(captions, max_length=lb.MAX_QUERY_LEN, padding="max_length" if lb.PAD_MAX else "longest",
                                               return_special_tokens_mask=True, return_tensors="pt", truncation=True)
        return {"input_ids": tok["input_ids"].to(device), "attention_mask": tok["attention_mask"].to(device)}

    def forward(self, images, targets=None, captions=None, positive_map=None, greenlight_map=None, tokenizer_input=None):
        """Training (with targets: GroundingTargets) -> {"loss_reg", "loss_centerness", "loss_cls", "loss_dot_product_token"}; eval ->
        Detections; positive_map: the reference's dict, or one map per sample as a list of B dicts or a PackedPositiveMaps on the device
        (phrase grounding, referring expressions).  greenlight_map is read by the MLM branch only and is accepted for signature parity."""
        if self.training and targets is None:
            raise ValueError("In training mode, targets should be passed")
        images, sizes = self._images_and_sizes(images)
        if tokenizer_input is None:
            if captions is None:
                raise ValueError("GeneralizedVLRCNN: captions (with a tokenizer) or tokenizer_input is required")
            tokenizer_input = self._tokenize(captions, images.device)
        visual_features, language_dict_features, _ = self.fusion_backbone(tokenizer_input, images)
        language_dict_features["mlm_labels"] = None
        if targets is not None and self.training:
            targets = targets.to(images.device)
        return self.rpn(sizes, list(visual_features), language_dict_features, positive_map, targets if self.training else None)

    @staticmethod
    def _images_and_sizes(images):
        """-> (the padded [B, 3, H, W] tensor, [(h, w)] per image as ImageList.image_sizes)"""
        sizes = None
        if isinstance(images, (tuple, list)):
            images, sizes = images
        elif hasattr(images, "tensors"):
            images, sizes = images.tensors, getattr(images, "image_sizes", None)
        if sizes is None:
            sizes = [tuple(images.shape[-2:])] * images.shape[0]     # (h, w) per image, as ImageList.image_sizes
        return images, sizes

    # ---- chunked open-vocabulary detection (TEST.CHUNKED_EVALUATION, engine/inference.py:483-575) ---------------------------------------
    # The reference runs the whole model once per (image, chunk of the vocabulary) and lets the evaluator sort the union.  Here the part of
    # the backbone that reads the image alone runs once per image, the part that reads the prompt alone once per evaluation, and only the
    # fused blocks, the FPN and the head run per pair; the chunks of an image are merged on the device (ops.det_merge).
    def encode_prompts(self, prompts):
        """prompts: detection_prompts.DetectionPrompts -> PromptState: the text prefix of all K prompts and the prompts on the device of the
        model.  Computed in eval mode under no_grad; nothing is cached here, the caller holds the state for as long as the weights stand."""
        if self.training:
            raise RuntimeError("encode_prompts: the model is in training mode (chunked detection is an inference path: call .eval())")
        prompts = prompts.to(next(self.parameters()).device)
        with torch.no_grad():
            text = self.fusion_backbone.text_prefix({"input_ids": prompts.input_ids, "attention_mask": prompts.attention_mask})
        return PromptState(text, prompts)

    def detect_chunked(self, images, prompt_state, prompts_per_pass=None, max_dets=None):
        """images as forward takes them; prompt_state: encode_prompts' result.  The K prompts are walked in passes of prompts_per_pass
        (default: all K at once; the last pass may be narrower): a pass runs the fused blocks, the FPN and the head on the pair batch whose
        sample b * P + p is (image b, prompt p of the pass), scoring the chunk's own classes only (C = the chunk width).  The K results
        per image are merged into one ranked list of at most max_dets (default K * DETECTIONS_PER_IMG) with the labels BoxAPEvaluator
        reads.  -> Detections with `chunk` set.  Nothing synchronises."""
        if self.training:
            raise RuntimeError("detect_chunked: the model is in training mode (chunked detection is an inference path: call .eval())")
        images, sizes = self._images_and_sizes(images)
        prompts, fb = prompt_state.prompts, self.fusion_backbone
        dev = images.device
        B, K, Cc = int(images.shape[0]), len(prompts), prompts.packed.num_classes
        if prompts.input_ids.device != dev:
            raise ValueError(f"detect_chunked: images on {dev}, the prompt state on {prompts.input_ids.device}")
        P = K if prompts_per_pass is None else int(prompts_per_pass)
        if P <= 0:
            raise ValueError(f"detect_chunked: prompts_per_pass {prompts_per_pass}")
        if not torch.is_tensor(sizes):
            sizes = torch.tensor([[float(w), float(h)] for h, w in sizes], dtype=torch.float32)
        sizes = sizes.to(device=dev, dtype=torch.float32, non_blocking=True)
        parts = []
        with torch.no_grad():
            image_state = fb.image_prefix(images)
            rows = torch.arange(B, device=dev)
            for k0 in range(0, K, P):
                p = min(P, K - k0)
                image_index = rows[:, None].expand(B, p).reshape(-1)              # (repeat_interleave would read its size back)
                text_index = torch.arange(k0, k0 + p, device=dev).repeat(B)
                visual, lang, _ = fb.fuse(image_state, prompt_state.text, image_index, text_index)
                lang["mlm_labels"] = None
                maps = PackedPositiveMaps(prompts.packed.class_ptr.index_select(0, text_index), prompts.packed.tok_idx)
                det = self.rpn(sizes.index_select(0, image_index), list(visual), lang, maps, None, num_classes=Cc)
                D = det.scores.shape[1]
                parts.append((det.boxes.view(B, p, D, 4), det.scores.view(B, p, D), det.labels.view(B, p, D), det.source.view(B, p, D),
                              det.count.view(B, p)))
            boxes, scores, labels, source, count = (torch.cat(col, dim=1) for col in zip(*parts))
            *merged, chunk, total = ops.det_merge(boxes, scores, labels, source, count, prompts.label_table, max_dets)
        return Detections(*merged, total, chunk=chunk)

    # ---- multi-scale test-time augmentation (TEST.USE_MULTISCALE, data/datasets/evaluation/box_aug.py) ---------------------------------
    # Every view (scale x flip) of every image runs the image side of the model; the un-cut candidates of all views are brought back to the
    # image's own frame (ops.det_aug_collect, one launch per view) and merged class by class on the device (ops.det_aug_merge).  The text
    # prefix does not depend on the view and is computed once.
    @staticmethod
    def multiscale_views(test_cfg):
        """-> [(scale, keep_range or None, flip)] in the reference's order: scale-major, un-flipped before flipped (box_aug.py:24-57)"""
        scales, ranges = list(test_cfg.SCALES), list(getattr(test_cfg, "RANGES", ()))
        if len(ranges) != len(scales):
            ranges = [None] * len(scales)
        views = []
        for scale, keep in zip(scales, ranges):
            keep = None if keep is None else (keep[0], keep[1])
            views.append((scale, keep, False))
            if getattr(test_cfg, "FLIP", False):
                views.append((scale, keep, True))
        return views

    def detect_multiscale(self, images, captions=None, positive_map=None, tokenizer_input=None, test_cfg=None):
        """images: a list of uint8 [H, W, 3] RGB device tensors, untransformed (as the reference's BBoxAugCollator hands them over);
        captions / tokenizer_input / positive_map as forward takes them; test_cfg (default cfg.TEST) is read for SCALES, RANGES,
        MAX_SIZE, FLIP, SPECIAL_NMS, TH, PRE_NMS_TOP_N, NUM_CLASSES and SELECT_CLASSES.  -> Detections of the fixed size
        [B, PRE_NMS_TOP_N] with boxes IN EACH IMAGE'S ORIGINAL FRAME and `view` set.  Eval mode only; nothing synchronises: every size
        comes from the images' shapes."""
        from ..data import DeviceDetectionTransform, det_resize_size
        if self.training:
            raise RuntimeError("detect_multiscale: the model is in training mode (multi-scale testing is an inference path: call .eval())")
        t = self.cfg.TEST if test_cfg is None else test_cfg
        top_n, mode = int(t.PRE_NMS_TOP_N), getattr(t, "SPECIAL_NMS", "none")
        if top_n <= 0:
            raise NotImplementedError("detect_multiscale: TEST.PRE_NMS_TOP_N <= 0 (no cut): the outputs have the fixed size [B, PRE_NMS_TOP_N]")
        if mode in ("soft-nms", "soft-vote"):
            raise NotImplementedError(f"detect_multiscale: TEST.SPECIAL_NMS {mode!r} is out of scope (\"vote\" and plain NMS are built)")
        mode = mode if mode == "vote" else "none"                # boxlist_nms: any other string is plain NMS
        views = self.multiscale_views(t)
        if not views:
            raise ValueError("detect_multiscale: TEST.SCALES is empty")
        select = [int(c) for c in getattr(t, "SELECT_CLASSES", ())]
        classes = sorted(set(select)) if select else list(range(1, int(t.NUM_CLASSES)))
        images = list(images)
        dev = images[0].device
        shapes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
        B = len(images)
        if tokenizer_input is None:
            if captions is None:
                raise ValueError("GeneralizedVLRCNN: captions (with a tokenizer) or tokenizer_input is required")
            tokenizer_input = self._tokenize(captions, dev)
        transform = DeviceDetectionTransform.for_views(self.cfg)
        fb = self.fusion_backbone
        per_view = []
        with torch.no_grad():
            d_classes = torch.tensor(classes, dtype=torch.int32).to(dev, non_blocking=True)
            text_state = fb.text_prefix(tokenizer_input)
            for scale, keep, flip in views:
                sizes = [det_resize_size(W, H, scale, getattr(t, "MAX_SIZE", None)) for H, W in shapes]
                batch = transform.apply(images, sizes, [flip] * B)
                visual, lang, _ = fb.fuse(fb.image_prefix(batch.tensors), text_state)
                lang["mlm_labels"] = None
                wh = torch.tensor([[float(ow), float(oh)] for oh, ow in batch.image_sizes], dtype=torch.float32).to(dev, non_blocking=True)
                cand = self.rpn(wh, list(visual), lang, positive_map, None, candidates=True)
                per_view.append((cand, ops.det_aug_view_rows(shapes, batch.image_sizes, flip, keep)))
            T = sum(int(cand[1].shape[1]) for cand, _ in per_view)
            out = (torch.empty((B, T, 4), dtype=torch.float32, device=dev), torch.empty((B, T), dtype=torch.float32, device=dev),
                   torch.empty((B, T), dtype=torch.int32, device=dev), torch.empty((B, T), dtype=torch.int32, device=dev),
                   torch.empty((B, T), dtype=torch.int32, device=dev))
            off = 0
            for v, (cand, rows) in enumerate(per_view):
                ops.det_aug_collect(*cand, rows, d_classes, out, off, v)
                off += int(cand[1].shape[1])
            *merged, view, count = ops.det_aug_merge(*out, d_classes, float(t.TH), mode, top_n)
        return Detections(*merged, count, view=view)


class PromptState:
    """encode_prompts' result: `text` (fusion_swin.TextState of the K prompts) and `prompts` (DetectionPrompts on the device)"""

    def __init__(self, text, prompts):
        self.text, self.prompts = text, prompts
