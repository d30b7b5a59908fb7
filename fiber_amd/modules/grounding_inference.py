"""Grounding inference of the fine-grained model on the MI355X kernels: VLDyHead's outputs -> boxes.

Mirrors fine_grained/maskrcnn_benchmark/modeling/rpn/vldyhead.py:917-1155 (VLDyHeadModule, eval side), modeling/rpn/inference.py:554-823
(ATSSPostProcessor, convert_grounding_to_od_logits[_v2], make_atss_postprocessor), modeling/rpn/anchor_generator.py:36-160 + :336-401
(AnchorGenerator, make_anchor_generator_complex, generate_anchors), modeling/box_coder.py:52-95 (decode) and csrc/cuda/ml_nms.cu.

The reference's path is host-bound: per level and image a nonzero, a data-dependent topk(k) and a boolean gather (each a device-to-host
synchronisation), then the N x N/64 suppression mask copied to the host and walked there.  Here every shape is fixed by the configuration:
  ops.det_scores   dense [B, A_l, C] scores, -1 where the candidate test fails            (csrc/detect.hip)
  torch.topk       per level with the FIXED k_l = min(pre_nms_top_n, A_l * C); -1 entries are padding
  ops.det_decode   decode + clip + small-box test, written into the level's slice of the concatenated [B, N] buffers, N = sum k_l
  torch.sort       per image, descending and stable, + one gather
  ops.nms_ml       mask kernel (one wave per 64 x 64 block) + select kernel (one wave per image, stops at detections_per_img)
so the whole of ATSSPostProcessor.forward can be captured in a hipGraph; Detections.to_list() is the only call that synchronises.
ATSSPostProcessor.candidates stops after the decode: multi-scale testing (GeneralizedVLRCNN.detect_multiscale) merges the candidates of
all views itself (ops.det_aug_collect, ops.det_aug_merge).

Deviations from the reference, each pinned by tests/test_detect_compare_host.py or tests/test_hip_detect.py:
  * the cut to detections_per_img takes the first D survivors in score order; the reference's kthvalue keeps every score >= the cut, i.e.
    more than D on an exact tie there.  Likewise exact ties across a top-k cut are broken by torch.topk, not by nonzero's order.
  * results come in descending score order (the reference returns ml_nms's index order).
  * suppression is strict IoU > NMS_TH as in ml_nms.cu (the reference's GPU path); its CPU nms uses >=.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from .. import lib, ops
from .vldyhead import VLDyHead

_UNSUPPORTED = {
    "token_logits": "the convolutional token head: FIBER scores with the dot-product logits",
    "box_cls": "classification-only scoring (no dot_product_logits): FIBER's grounding head always returns them",
    "POWER": "DYHEAD.SCORE_AGG POWER: no FIBER config sets it (MEAN and MAX are built)",
    "ONEHOT": "DYHEAD.SCORE_AGG ONEHOT: no FIBER config sets it (MEAN and MAX are built)",
    "bbox_aug": "bbox_aug_enabled / bbox_aug_vote change what forward returns (the candidates before select_over_all_levels); a "
                "post-processor here keeps one return contract: multi-scale testing (TEST.USE_MULTISCALE) calls candidates() instead, "
                "through GeneralizedVLRCNN.detect_multiscale",
    "nms_thresh": "NMS_TH <= 0 (boxlist_ml_nms returns its input): every FIBER config suppresses",
    "num_anchors": "one anchor per position: the dot product pairs ONE 256-channel feature with the tokens (vldyhead.py:861-865)",
}


# ---- anchors (anchor_generator.py:336-401: the classic generate_anchors, restated) ------------------------------------------------------
def _whctrs(anchor):
    w = anchor[2] - anchor[0] + 1
    h = anchor[3] - anchor[1] + 1
    return w, h, anchor[0] + 0.5 * (w - 1), anchor[1] + 0.5 * (h - 1)


def _mkanchors(ws, hs, x_ctr, y_ctr):
    ws, hs = ws[:, None], hs[:, None]
    return np.hstack((x_ctr - 0.5 * (ws - 1), y_ctr - 0.5 * (hs - 1), x_ctr + 0.5 * (ws - 1), y_ctr + 0.5 * (hs - 1)))


def generate_anchors(stride=16, sizes=(32, 64, 128, 256, 512), aspect_ratios=(0.5, 1, 2)):
    """Cell anchors (x1, y1, x2, y2) centred on stride / 2: every aspect ratio of the (0, 0, stride - 1, stride - 1) window, each at
    every scale sizes / stride.  fp64 numpy, as the reference."""
    scales = np.array(sizes, dtype=float) / stride
    ratios = np.array(aspect_ratios, dtype=float)
    base = np.array([1, 1, stride, stride], dtype=float) - 1
    w, h, x_ctr, y_ctr = _whctrs(base)
    ws = np.round(np.sqrt(w * h / ratios))
    hs = np.round(ws * ratios)
    by_ratio = _mkanchors(ws, hs, x_ctr, y_ctr)
    out = []
    for a in by_ratio:
        w, h, x_ctr, y_ctr = _whctrs(a)
        out.append(_mkanchors(w * scales, h * scales, x_ctr, y_ctr))
    return torch.from_numpy(np.vstack(out))


class AnchorGenerator(nn.Module):
    """anchor_generator.py:36-121.  grid_anchors(grid_sizes) -> one fp32 [A_l, 4] tensor per level (position-major, cell anchors inner),
    cached by (level, grid size, device).  The anchors do not depend on the image: the per-image BoxList copies of the reference (and
    their "visibility" field, which inference never reads) are not built."""

    def __init__(self, sizes=(128, 256, 512), aspect_ratios=(0.5, 1.0, 2.0), anchor_strides=(8, 16, 32), straddle_thresh=0):
        super().__init__()
        if len(anchor_strides) == 1:
            cell = [generate_anchors(anchor_strides[0], sizes, aspect_ratios).float()]
        else:
            if len(anchor_strides) != len(sizes):
                raise RuntimeError("FPN should have #anchor_strides == #sizes")
            cell = [generate_anchors(s, z if isinstance(z, (tuple, list)) else (z,), aspect_ratios).float()
                    for s, z in zip(anchor_strides, sizes)]
        self.strides = anchor_strides
        self.cell_anchors = cell
        self.straddle_thresh = straddle_thresh
        self._cache = {}

    def num_anchors_per_location(self):
        return [len(c) for c in self.cell_anchors]

    def grid_anchors(self, grid_sizes, device="cpu"):
        out = []
        for l, (size, stride, base) in enumerate(zip(grid_sizes, self.strides, self.cell_anchors)):
            key = (l, int(size[0]), int(size[1]), str(device))
            if key not in self._cache:
                gh, gw = int(size[0]), int(size[1])
                sx = torch.arange(0, gw * stride, step=stride, dtype=torch.float32)
                sy = torch.arange(0, gh * stride, step=stride, dtype=torch.float32)
                yy, xx = torch.meshgrid(sy, sx, indexing="ij")
                xx, yy = xx.reshape(-1), yy.reshape(-1)
                shifts = torch.stack((xx, yy, xx, yy), dim=1)
                self._cache[key] = (shifts.view(-1, 1, 4) + base.view(1, -1, 4)).reshape(-1, 4).contiguous().to(device)
            out.append(self._cache[key])
        return out

    def forward(self, feature_maps):
        return self.grid_anchors([f.shape[-2:] for f in feature_maps], feature_maps[0].device)


def make_anchor_generator_complex(config):
    """anchor_generator.py:138-160"""
    r = config.MODEL.RPN
    if r.USE_FPN:
        assert len(r.ANCHOR_STRIDE) == len(r.ANCHOR_SIZES), "Only support FPN now"
        sizes = tuple(tuple(r.OCTAVE ** (s / float(r.SCALES_PER_OCTAVE)) * size for s in range(r.SCALES_PER_OCTAVE)) for size in r.ANCHOR_SIZES)
    else:
        assert len(r.ANCHOR_STRIDE) == 1, "Non-FPN should have a single ANCHOR_STRIDE"
        sizes = r.ANCHOR_SIZES
    return AnchorGenerator(sizes, r.ASPECT_RATIOS, r.ANCHOR_STRIDE, r.STRADDLE_THRESH)


class BoxCoder:
    """box_coder.py:7-95, decode only (plain torch; the inference path decodes in ops.det_decode, which hard-wires the grounding
    head's weights (10, 10, 5, 5) and clamp).  vldyhead.py:54-115's BoxCoder(cfg) is the same map written around (x1 + x2) / 2: the two
    differ in rounding only."""

    def __init__(self, weights=(10.0, 10.0, 5.0, 5.0), bbox_xform_clip=math.log(1000.0 / 16)):
        self.weights = tuple(float(w) for w in weights)
        self.bbox_xform_clip = bbox_xform_clip

    def decode(self, rel_codes, boxes):
        boxes = boxes.to(rel_codes.dtype)
        widths = boxes[:, 2] - boxes[:, 0] + 1
        heights = boxes[:, 3] - boxes[:, 1] + 1
        ctr_x = boxes[:, 0] + 0.5 * widths
        ctr_y = boxes[:, 1] + 0.5 * heights
        wx, wy, ww, wh = self.weights
        dx, dy = rel_codes[:, 0::4] / wx, rel_codes[:, 1::4] / wy
        dw = torch.clamp(rel_codes[:, 2::4] / ww, max=self.bbox_xform_clip)
        dh = torch.clamp(rel_codes[:, 3::4] / wh, max=self.bbox_xform_clip)
        pcx, pcy = dx * widths[:, None] + ctr_x[:, None], dy * heights[:, None] + ctr_y[:, None]
        pw, ph = torch.exp(dw) * widths[:, None], torch.exp(dh) * heights[:, None]
        out = torch.zeros_like(rel_codes)
        out[:, 0::4], out[:, 1::4] = pcx - 0.5 * pw, pcy - 0.5 * ph
        out[:, 2::4], out[:, 3::4] = pcx + 0.5 * pw - 1, pcy + 0.5 * ph - 1
        return out


def positive_map_to_csr(positive_map, num_classes, v2=False):
    """The reference's {label: [token positions] | int} -> (class_ptr int32 [C + 1], tok_idx int32 [nnz]) with class = label - 1 (both
    convert_grounding_to_od_logits and _v2 with disable_minus_one=False).  v2 accepts int entries; labels outside [1, C] are an error
    (the reference would index out of range)."""
    rows = [[] for _ in range(num_classes)]
    for label, toks in positive_map.items():
        if isinstance(toks, int):
            if not v2:
                raise TypeError("positive_map: int entries are the MDETR-style (v2) form")
            toks = [toks]
        c = int(label) - 1
        if not 0 <= c < num_classes:
            raise ValueError(f"positive_map: label {label} outside 1..{num_classes}")
        toks = [int(t) for t in toks]
        if any(t < 0 or t >= 256 for t in toks):
            raise ValueError(f"positive_map: token position outside 0..255 for label {label}")
        rows[c] = toks                                      # a repeated label overwrites, as the reference's assignment does
    ptr = np.zeros(num_classes + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    idx = np.array([t for r in rows for t in r], dtype=np.int32)
    return torch.from_numpy(ptr), torch.from_numpy(idx if idx.size else np.zeros(1, dtype=np.int32))


class PackedPositiveMaps:
    """One positive map per sample: class_ptr int32 [B, C + 1] (row b: absolute offsets of sample b's classes into tok_idx) and the
    samples' token lists concatenated in tok_idx int32 [nnz].  What ATSSPostProcessor.forward takes in place of a dict when every
    image has its own caption; already on the device, it costs no copy, so the call can be captured in a graph."""

    def __init__(self, class_ptr, tok_idx):
        self.class_ptr, self.tok_idx = class_ptr, tok_idx

    @property
    def num_classes(self):
        return int(self.class_ptr.shape[1]) - 1

    def __len__(self):
        return int(self.class_ptr.shape[0])

    def to(self, device):
        """Both tensors travel in ONE copy (class_ptr padded to a multiple of 16 bytes, then tok_idx)."""
        have, want = self.class_ptr.device, torch.device(device)
        if have.type == want.type and want.index in (None, have.index):
            return self
        n = self.class_ptr.numel()
        pad = -n % 4
        flat = torch.cat([self.class_ptr.reshape(-1), self.class_ptr.new_zeros(pad), self.tok_idx.reshape(-1)]).to(device)
        return PackedPositiveMaps(flat[:n].view(self.class_ptr.shape), flat[n + pad:])


def pack_positive_maps(maps, num_classes, v2=False):
    """A list of B reference-form dicts (positive_map_to_csr's validation applies to each) -> PackedPositiveMaps on the host.  Classes a
    sample does not use have empty rows, which score -1: top-k, decode and `source` keep their meaning with the padded num_classes."""
    if isinstance(maps, dict) or len(maps) == 0:
        raise ValueError("pack_positive_maps: a non-empty list of positive maps, one per sample")
    ptrs, idxs, off = [], [], 0
    for m in maps:
        ptr, idx = positive_map_to_csr(m, num_classes, v2)
        nnz = int(ptr[-1])
        ptrs.append(ptr + off)
        idxs.append(idx[:nnz])
        off += nnz
    idx = torch.cat(idxs)
    return PackedPositiveMaps(torch.stack(ptrs).contiguous(), idx if idx.numel() else torch.zeros(1, dtype=torch.int32))


class Detections:
    """Fixed-size result: boxes fp32 [B, D, 4] (xyxy, +1 convention), scores fp32 [B, D] (-1 past count), labels int32 [B, D],
    source int32 [B, D] (level << 28 | anchor << 10 | class; -1 past count), count int32 [B]; descending score per image.  chunk int32
    [B, D] (the prompt a detection came from, -1 past count; its source's class field is local to that prompt) is set by chunked detection
    (GeneralizedVLRCNN.detect_chunked) only, None otherwise.  view int32 [B, D] (the view of multi-scale testing a detection came from,
    scale-major, un-flipped before flipped; -1 past count; for a voted cluster `source` and `view` are its leader's) is set by
    GeneralizedVLRCNN.detect_multiscale only, None otherwise."""
    SOURCE_A_SHIFT, SOURCE_LEVEL_SHIFT = 10, 28

    def __init__(self, boxes, scores, labels, source, count, chunk=None, view=None):
        self.boxes, self.scores, self.labels, self.source, self.count, self.chunk = boxes, scores, labels, source, count, chunk
        self.view = view

    def to_list(self):
        """Per image {"boxes", "scores", "labels" (int64), "source"} trimmed to count.  The one call that synchronises."""
        n = self.count.cpu().tolist()
        return [{"boxes": self.boxes[b, :k], "scores": self.scores[b, :k], "labels": self.labels[b, :k].long(), "source": self.source[b, :k]}
                for b, k in enumerate(n)]


class ATSSPostProcessor(nn.Module):
    """inference.py:554-738 for the dot-product grounding path."""

    def __init__(self, pre_nms_thresh, pre_nms_top_n, nms_thresh, fpn_post_nms_top_n, min_size, num_classes, box_coder,
                 bbox_aug_enabled=False, bbox_aug_vote=False, score_agg="MEAN", mdetr_style_aggregate_class_num=-1):
        super().__init__()
        if bbox_aug_enabled or bbox_aug_vote:
            raise NotImplementedError(f"ATSSPostProcessor bbox_aug: {_UNSUPPORTED['bbox_aug']}")
        if score_agg in ("POWER", "ONEHOT"):
            raise NotImplementedError(f"ATSSPostProcessor: {_UNSUPPORTED[score_agg]}")
        if score_agg not in ("MEAN", "MAX"):
            raise NotImplementedError(f"ATSSPostProcessor score_agg {score_agg!r}")
        if not nms_thresh > 0:
            raise NotImplementedError(f"ATSSPostProcessor: {_UNSUPPORTED['nms_thresh']}")
        if not fpn_post_nms_top_n > 0:
            raise NotImplementedError("ATSSPostProcessor DETECTIONS_PER_IMG <= 0 (no cut): the outputs have the fixed size [B, D]")
        if tuple(box_coder.weights) != (10.0, 10.0, 5.0, 5.0) or abs(box_coder.bbox_xform_clip - math.log(1000.0 / 16)) > 1e-12:
            raise NotImplementedError("ATSSPostProcessor: the decode kernel hard-wires BoxCoder((10, 10, 5, 5)) and the log(1000/16) clamp")
        self.pre_nms_thresh, self.pre_nms_top_n, self.nms_thresh = pre_nms_thresh, pre_nms_top_n, nms_thresh
        self.fpn_post_nms_top_n, self.min_size, self.num_classes = fpn_post_nms_top_n, min_size, num_classes
        self.box_coder, self.score_agg = box_coder, score_agg
        self.mdetr_style_aggregate_class_num = mdetr_style_aggregate_class_num
        self._csr = {}

    def num_score_classes(self, box_cls=None):
        """Width C of the dense scores: num_class of the v2 mapping, else box_cls's channel count (num_anchors = 1) or num_classes - 1."""
        if self.mdetr_style_aggregate_class_num != -1:
            return int(self.mdetr_style_aggregate_class_num)
        if box_cls is not None:
            return int(box_cls[0].shape[1])
        return int(self.num_classes) - 1

    CSR_CACHE = 16                                          # maps kept on the device (least recently used goes first)

    def csr(self, positive_map, C, device):
        """CSR form of the positive map on `device`.  The last CSR_CACHE distinct (map, C, device) are kept, so a detection prompt costs
        its host-to-device copy once while referring-expression evaluation (a new map per sample) does not grow without bound.  A map
        seen for the first time is copied here, inside forward: a graph capture needs the map to have been seen before (one eager
        call, or this method) and `image_sizes` given as a device tensor."""
        v2 = self.mdetr_style_aggregate_class_num != -1
        key = (tuple(sorted((int(k), v if isinstance(v, int) else tuple(int(t) for t in v)) for k, v in positive_map.items())), C, str(device))
        hit = self._csr.pop(key, None)
        if hit is None:
            ptr, idx = positive_map_to_csr(positive_map, C, v2)
            hit = (ptr.to(device), idx.to(device))
            while len(self._csr) >= self.CSR_CACHE:
                self._csr.pop(next(iter(self._csr)))
        self._csr[key] = hit                                 # (dicts keep insertion order: re-inserting marks it most recently used)
        return hit

    def level_k(self, num_anchors, C):
        return min(int(self.pre_nms_top_n), num_anchors * C)

    def candidates(self, box_regression, centerness, image_sizes, anchors, dot_product_logits=None, positive_map=None, box_cls=None,
                   token_logits=None, num_classes=None):
        """forward up to and including the per-level decode (arguments as forward takes them) -> (boxes fp32 [B, N, 4], scores fp32
        [B, N], labels int32 [B, N], source int32 [B, N]), N = sum of the levels' fixed k: the decoded, clipped top-k of every level,
        concatenated in level order, padding under score -1; no sort, no NMS, no cut.  What the reference's post-processor returns with
        bbox_aug_enabled (inference.py:708), in fixed shapes."""
        if token_logits is not None:
            raise NotImplementedError(f"ATSSPostProcessor token_logits: {_UNSUPPORTED['token_logits']}")
        if dot_product_logits is None:
            raise NotImplementedError(f"ATSSPostProcessor box_cls only: {_UNSUPPORTED['box_cls']}")
        if positive_map is None:
            raise ValueError("ATSSPostProcessor: positive_map is required (without one every score is 0 in the reference)")
        if box_regression[0].shape[1] != 4:
            raise NotImplementedError(f"ATSSPostProcessor num_anchors != 1: {_UNSUPPORTED['num_anchors']}")
        dev = dot_product_logits[0].device
        B = dot_product_logits[0].shape[0]
        C = self.num_score_classes(box_cls) if num_classes is None else int(num_classes)
        if isinstance(positive_map, (list, tuple)):
            if len(positive_map) != B:
                raise ValueError(f"ATSSPostProcessor: {len(positive_map)} positive maps for a batch of {B}")
            positive_map = pack_positive_maps(positive_map, C, self.mdetr_style_aggregate_class_num != -1).to(dev)
        if isinstance(positive_map, PackedPositiveMaps):
            if len(positive_map) != B or positive_map.num_classes != C or positive_map.class_ptr.device != dev:
                raise ValueError(f"ATSSPostProcessor: packed positive maps {tuple(positive_map.class_ptr.shape)} on "
                                 f"{positive_map.class_ptr.device} for a batch of {B} with {C} classes on {dev}")
            ptr, idx = positive_map.class_ptr, positive_map.tok_idx
        else:
            ptr, idx = self.csr(positive_map, C, dev)
        ks = [self.level_k(d.shape[1], C) for d in dot_product_logits]
        N = sum(ks)
        if N > lib.plain("fiber_det_max_candidates"):
            raise lib.FiberHipError(f"ATSSPostProcessor: {N} candidates per image exceed the select kernel's {lib.plain('fiber_det_max_candidates')}")
        out = (torch.empty((B, N, 4), dtype=torch.float32, device=dev), torch.empty((B, N), dtype=torch.float32, device=dev),
               torch.empty((B, N), dtype=torch.int32, device=dev), torch.empty((B, N), dtype=torch.int32, device=dev))
        off = 0
        for l, (reg, ctr, anc, dot, k) in enumerate(zip(box_regression, centerness, anchors, dot_product_logits, ks)):
            dense = ops.det_scores(dot, ctr, ptr, idx, self.pre_nms_thresh, self.score_agg)
            val, flat = torch.topk(dense.view(B, -1), k, dim=1)
            ops.det_decode(val, flat, reg, anc, image_sizes, out, off, l, C, self.min_size)
            off += k
        return out

    def forward(self, box_regression, centerness, image_sizes, anchors, dot_product_logits=None, positive_map=None, box_cls=None,
                token_logits=None, num_classes=None):
        """box_regression / centerness / dot_product_logits: per level, as VLDyHead.forward returns them; image_sizes fp32 [B, 2] device
        tensor of (w, h) per image; anchors: one [A_l, 4] tensor per level (AnchorGenerator.grid_anchors of the feature shapes: the
        reference's per-image BoxList copies differ in nothing but the size field).  positive_map: the reference's dict (one map for the
        batch, cached by csr()), a list of B dicts (one per sample: packed here with one host-to-device copy per call, not cached), or a
        PackedPositiveMaps already on the device (no copy).  num_classes: the width C of the dense scores for this call (chunked detection
        scores one prompt's classes at a time); None = num_score_classes().  -> Detections"""
        boxes, scores, labels, source = self.candidates(box_regression, centerness, image_sizes, anchors, dot_product_logits, positive_map,
                                                        box_cls, token_logits, num_classes)
        scores, order = torch.sort(scores, dim=1, descending=True, stable=True)
        boxes = torch.gather(boxes, 1, order[:, :, None].expand(-1, -1, 4))
        labels, source = torch.gather(labels, 1, order), torch.gather(source, 1, order)
        return Detections(*ops.nms_ml(boxes, scores, labels, source, self.nms_thresh, self.fpn_post_nms_top_n))


def make_atss_postprocessor(config, box_coder, is_train=False):
    """inference.py:798-823.  TEST.USE_MULTISCALE is not forwarded into bbox_aug_enabled: the switch selects
    GeneralizedVLRCNN.detect_multiscale, which asks the same post-processor for its candidates()."""
    a = config.MODEL.ATSS
    return ATSSPostProcessor(
        pre_nms_thresh=a.INFERENCE_TH_TRAIN if is_train else a.INFERENCE_TH,
        pre_nms_top_n=a.PRE_NMS_TOP_N_TRAIN if is_train else a.PRE_NMS_TOP_N,
        nms_thresh=a.NMS_TH,
        fpn_post_nms_top_n=a.POST_NMS_TOP_N_TRAIN if is_train else a.DETECTIONS_PER_IMG,
        min_size=0, num_classes=a.NUM_CLASSES, box_coder=box_coder,
        score_agg=config.MODEL.DYHEAD.SCORE_AGG, mdetr_style_aggregate_class_num=config.TEST.MDETR_STYLE_AGGREGATE_CLASS_NUM)


class VLDyHeadModule(nn.Module):
    """vldyhead.py:917-1155: head (checkpoint keys `head.*`) + anchors + box selector (eval) / loss evaluator (training with targets)."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.head = VLDyHead(cfg)
        self.box_selector_test = make_atss_postprocessor(cfg, BoxCoder(), is_train=False)
        self.anchor_generator = make_anchor_generator_complex(cfg)
        if any(n != 1 for n in self.anchor_generator.num_anchors_per_location()):
            raise NotImplementedError(f"VLDyHeadModule: {_UNSUPPORTED['num_anchors']}")
        self._loss_evaluator = None                          # grounding_train.ATSSLossComputation, built by the first training step

    def _train(self, features, language_dict_features, targets):
        """vldyhead.py:1022-1105 with RPN_ONLY: the reference's loss dict; targets: grounding_train.GroundingTargets on the device."""
        from .grounding_train import ATSSLossComputation
        if self._loss_evaluator is None:
            self._loss_evaluator = ATSSLossComputation(self.cfg)
        h = self.head
        logits, bbox_reg, centerness, q, proj, tbias = h.training_outputs(features, language_dict_features["embedded"])
        cls, reg, ctr, token = self._loss_evaluator(logits, bbox_reg, centerness, targets, self.anchor_generator(features), q, proj, tbias,
                                                    h.log_scale, language_dict_features.get("masks"))
        w = getattr(self.cfg.MODEL.DYHEAD.FUSE_CONFIG, "DOT_PRODUCT_TOKEN_LOSS_WEIGHT", 1.0)
        return {"loss_reg": reg, "loss_centerness": ctr, "loss_cls": cls, "loss_dot_product_token": token * w}

    def forward(self, image_sizes, features, language_dict_features, positive_map=None, targets=None, num_classes=None, candidates=False):
        """Training mode with `targets`: -> {"loss_reg", "loss_centerness", "loss_cls", "loss_dot_product_token"} (image_sizes and
        positive_map are not read: the anchors do not depend on the image and the targets carry their positive map).  Eval: image_sizes: [(h, w)] per image as ImageList.image_sizes, or a [B, 2] tensor of (w, h); features: the FPN levels
        [B, C, H, W]; language_dict_features["embedded"]: [B, 256, LANG_DIM]; positive_map: one dict for the batch, a list of B dicts or a
        PackedPositiveMaps (one map per sample: see ATSSPostProcessor.forward).  -> Detections.  A list of sizes is copied to the device
        here (a host-to-device copy per call); pass the tensor, already on the device, to avoid it or to capture the call in a graph.
        num_classes: see ATSSPostProcessor.forward.  candidates=True (eval only): -> ATSSPostProcessor.candidates' (boxes, scores, labels,
        source) instead of Detections (multi-scale testing merges the views' candidates itself)."""
        if self.training:
            if targets is None:
                raise NotImplementedError("VLDyHeadModule in training mode needs targets= (grounding_train.pack_targets); without them "
                                          "it is the inference side")
            return self._train(features, language_dict_features, targets)
        dev = features[0].device
        if not torch.is_tensor(image_sizes):
            image_sizes = torch.tensor([[float(w), float(h)] for h, w in image_sizes], dtype=torch.float32)
        image_sizes = image_sizes.to(device=dev, dtype=torch.float32)
        with torch.no_grad():
            out = self.head(features, language_dict_features, language_dict_features["embedded"])
            post = self.box_selector_test.candidates if candidates else self.box_selector_test
            return post(out[1], out[2], image_sizes, self.anchor_generator(features), out[6], positive_map, box_cls=out[0],
                        token_logits=out[3], num_classes=num_classes)
