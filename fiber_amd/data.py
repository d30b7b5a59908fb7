"""On-device input pipeline: the reference's per-sample CPU transforms, executed on the GPU after
the H2D copy of the RAW sample bytes.

  * `DeviceImageTransform` = `albef_transform(size)` of coarse_grained/fiber/transforms/transform.py:10-17 (PIL bicubic Resize ->
    ToTensor -> Normalize), bit-identical to PIL + torchvision on uint8 RGB input (csrc/input.hip restates Pillow's resampler);
  * `DeviceRandAugTransform` = `albef_transform_randaug(size)` of transform.py:20-45, the TRAINING transform of every configuration
    (RandomResizedCrop -> RandomHorizontalFlip -> RandomAugment(2, 7) -> ToTensor -> Normalize): `plan` draws on the host, `apply` runs
    7 kernels on the device; `keys_to_transforms` maps config["train_transform_keys"] / ["val_transform_keys"] to the two transforms;
  * `mlm_mask` = the masking rule of `DataCollatorForLanguageModeling(mlm_probability)` used by BaseDataModule
    (datamodules/datamodule_base.py:52) -> `text_ids_mlm`, `text_labels_mlm` of the batch schema (base_dataset.py:223-243).

  * `DeviceDetectionTransform` / `device_collate_grounding` = the fine-grained model's `build_transforms` (Resize(min, max) with PIL
    BILINEAR -> RandomHorizontalFlip -> ToTensor -> Normalize(format)), `BoxList.resize` / `transpose`, `to_image_list(size_divisible)`
    and `BatchCollator`, for the configuration every FIBER yaml uses: one ragged batch of raw uint8 images -> the padded
    [B, 3, Hp, Wp] tensor GeneralizedVLRCNN.forward consumes, its GroundingTargets and its tokenizer_input.

What stays on the host: JPEG decode (`Image.open(...).convert("RGB")`, base_dataset.py:97-103) and tokenisation -- the loader
workers hand over uint8 [H, W, 3] arrays and int64 token ids; everything after that is stream-ordered device work, so at
~800 images/s per GPU the loader no longer resizes and normalises 2 x 384^2 fp32 images per sample on CPU cores.
"""
import math

import numpy as np
import torch

from . import lib, ops

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)

_DESC = np.dtype([("src", "<i8"), ("H", "<i4"), ("W", "<i4"), ("src_stride", "<i4"), ("ksize_h", "<i4"), ("ksize_v", "<i4"),
                  ("tmp_off", "<i4"), ("coef_h_off", "<i4"), ("coef_v_off", "<i4")])
assert _DESC.itemsize == 40
_DET_DESC = np.dtype([("src", "<i8"), ("H", "<i4"), ("W", "<i4"), ("src_stride", "<i4"), ("oh", "<i4"), ("ow", "<i4"), ("ksize_h", "<i4"),
                      ("ksize_v", "<i4"), ("tmp_off", "<i4"), ("coef_h_off", "<i4"), ("coef_v_off", "<i4"), ("flip", "<i4"),
                      ("tmp_pitch", "<i4")])
assert _DET_DESC.itemsize == 56
_BOX_PARAM = np.dtype([("ratio_w", "<f4"), ("ratio_h", "<f4"), ("flip", "<i4"), ("new_w", "<f4"), ("num_gt", "<i4")])
assert _BOX_PARAM.itemsize == 20
_M64 = (1 << 64) - 1


class DeviceImageTransform:
    """images: list of uint8 [H, W, 3] tensors on a HIP device (ragged sizes) -> fp32 [B, 3, size, size]."""

    def __init__(self, size=384, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        self.size = int(size)
        self.mean = (lib.C.c_float * 3)(*mean)
        self.std = (lib.C.c_float * 3)(*std)

    def __call__(self, images):
        S, n = self.size, len(images)
        dev = images[0].device
        desc = np.zeros(n, _DESC)
        tmp_off = coef_off = 0
        for i, im in enumerate(images):
            if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or im.stride(2) != 1 or im.stride(1) != 3:
                raise ValueError("DeviceImageTransform needs uint8 [H, W, 3] images with packed pixels")
            H, W = int(im.shape[0]), int(im.shape[1])
            kh, kv = lib.plain("fiber_resample_ksize", W, S), lib.plain("fiber_resample_ksize", H, S)
            desc[i] = (lib.ptr(im), H, W, int(im.stride(0)), kh, kv, tmp_off, coef_off, coef_off + S * (2 + kh))
            tmp_off += (H * S * 3 + 15) // 16 * 16
            coef_off += S * (2 + kh) + S * (2 + kv)
        if tmp_off >= 2 ** 31:
            raise ValueError("batch too large for one call (intermediate images exceed 2 GiB): split it")
        d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev, non_blocking=True)
        coef = torch.empty(coef_off, dtype=torch.int32, device=dev)
        tmp = torch.empty(tmp_off, dtype=torch.uint8, device=dev)
        out = torch.empty((n, 3, S, S), dtype=torch.float32, device=dev)
        lib.call("fiber_resize_bicubic_norm_u8", lib.ptr(d_desc), n, lib.ptr(coef), lib.ptr(tmp), lib.ptr(out), S,
                 int(desc["H"].max()), self.mean, self.std)
        self._keep = (images, d_desc)          # the sources / table must outlive the (asynchronous) kernels of this call
        return out


def mlm_mask(ids, seed=None, mlm_probability=0.15, mask_id=50264, vocab=50265, special=(0, 2)):
    """ids int64 [B, S] (device) -> (text_ids_mlm, text_labels_mlm).  `special`: inclusive id range never masked (RoBERTa
    <s> = 0, <pad> = 1, </s> = 2).  `seed`: 64-bit key of this batch (default: the next key of the input pipeline's own stream,
    ops.collate_seed(): by value and advancing per batch whether or not the training step is a captured hipGraph)."""
    ids = ids.contiguous()
    out, lab = torch.empty_like(ids), torch.empty_like(ids)
    if seed is None:
        seed = ops.collate_seed()
    lib.call("fiber_mlm_mask_i64", lib.ptr(ids), lib.ptr(out), lib.ptr(lab), ids.numel(), int(seed) & (2 ** 64 - 1),
             int(mlm_probability * 2 ** 32), int(mask_id), int(vocab), int(special[0]), int(special[1]))
    return out, lab


def device_collate(samples, transform, seed=None, max_text_len=40, pad_id=1, draw_false_image=0):
    """The device-side half of BaseDataset.collate (base_dataset.py:172-245) for RAW samples: each sample is a dict with
    `image` (uint8 [H, W, 3] device tensor), optional `false_image_0`, and `text_ids` (1-D int64 device tensor, already
    tokenised with <s> ... </s>).  Returns the batch dict FIBERTransformerSS.forward consumes."""
    dev = samples[0]["image"].device
    B = len(samples)
    ids = torch.full((B, max_text_len), pad_id, dtype=torch.int64, device=dev)
    for i, s in enumerate(samples):
        t = s["text_ids"][:max_text_len]
        ids[i, :t.numel()] = t
    ids_mlm, labels_mlm = mlm_mask(ids, seed)
    batch = {"image": [transform([s["image"] for s in samples])], "text": ["" for _ in samples], "text_ids": ids,
             "text_masks": (ids != pad_id).long(), "text_labels": torch.full_like(ids, -100), "text_ids_mlm": ids_mlm,
             "text_labels_mlm": labels_mlm}
    for k in range(draw_false_image):
        batch[f"false_image_{k}"] = [transform([s[f"false_image_{k}"] for s in samples])]
    return batch


# ---- the fine-grained (grounding) model's input ----------------------------------------------------------------------------------------
def _need(cond, name, why):
    if not cond:
        raise NotImplementedError(f"{name}: {why}")


def hash_u32(seed, idx):
    """csrc/common.h hash_u32 on the host (splitmix64 finaliser of seed + idx * golden ratio, high 32 bits)."""
    z = (seed + idx * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return (z ^ (z >> 31)) >> 32


def det_resize_size(w, h, size, max_size):
    """Resize.get_size of fine_grained/maskrcnn_benchmark/data/transforms/transforms.py:94-116 for one drawn `size` -> (oh, ow)."""
    if max_size is not None:
        min_original_size = float(min((w, h)))
        max_original_size = float(max((w, h)))
        if max_original_size / min_original_size * size > max_size:
            size = int(round(max_size * min_original_size / max_original_size))
    if (w <= h and w == size) or (h <= w and h == size):
        return (h, w)
    if w < h:
        ow = size
        oh = int(size * h / w)
    else:
        oh = size
        ow = int(size * w / h)
    return (oh, ow)


def _box_table(rows, dev):
    """rows: (ratio_w, ratio_h, flip, new_w, num_gt) per image -> the device table of fiber_det_boxes_f32"""
    t = np.zeros(len(rows), _BOX_PARAM)
    for i, r in enumerate(rows):
        t[i] = r
    return torch.from_numpy(t.view(np.uint8).copy()).to(dev, non_blocking=True)


class DetImageList:
    """What DeviceDetectionTransform returns (the reference's ImageList plus the bookkeeping of its BoxLists): `tensors` fp32
    [B, 3, Hp, Wp], `image_sizes` [(oh, ow)] and `original` [(orig_h, orig_w, flipped)] per image, all but `tensors` on the host."""

    def __init__(self, tensors, image_sizes, original):
        self.tensors, self.image_sizes, self.original = tensors, image_sizes, original

    def to(self, device):
        return DetImageList(self.tensors.to(device), self.image_sizes, self.original)

    def box_params(self, num_gt):
        """The forward table (original frame -> resized, flipped frame): the ratios of BoxList.resize (bounding_box.py:109), in double,
        rounded to fp32 as the reference's tensor * python-float products round them."""
        return [(float(ow) / float(W), float(oh) / float(H), int(f), float(ow), int(n))
                for (oh, ow), (H, W, f), n in zip(self.image_sizes, self.original, num_gt)]

    def boxes_to_original(self, detections):
        """Detections (or a [B, D, 4] box tensor) in the resized frame -> boxes fp32 [B, D, 4] in each image's original frame: the
        `prediction.resize((orig_w, orig_h))` of the reference's inference loop (engine/inference.py:308), with BoxList.resize's ratio rule.
        No flip is undone: evaluation never flips."""
        boxes = getattr(detections, "boxes", detections)
        if boxes.dim() != 3 or boxes.shape[0] != len(self.image_sizes) or boxes.shape[2] != 4:
            raise ValueError(f"boxes_to_original: boxes {tuple(boxes.shape)} for {len(self.image_sizes)} images")
        out = boxes.float().clone(memory_format=torch.contiguous_format)
        D = int(out.shape[1])
        rows = [(float(W) / float(ow), float(H) / float(oh), 0, float(W), D) for (oh, ow), (H, W, _) in zip(self.image_sizes, self.original)]
        table = _box_table(rows, out.device)
        lib.call("fiber_det_boxes_f32", lib.ptr(out), lib.ptr(table), len(rows), D)
        self._keep = table
        return out


class DeviceDetectionTransform:
    """`build_transforms(cfg, is_train)` of fine_grained/maskrcnn_benchmark/data/transforms/build.py:5-43 plus `to_image_list(...,
    DATALOADER.SIZE_DIVISIBILITY)` on the device.  images: list of uint8 [H, W, 3] RGB device tensors (ragged, row-strided views
    allowed); seed: the 64-bit key of this batch (default ops.collate_seed()).  -> DetImageList.

    The size choice and the flip are drawn on the host (the batch shape depends on them) and are a pure function of (seed, sample
    index i): hash_u32(seed, 2 i) % len(min_size) picks the size (random.choice in the reference), hash_u32(seed, 2 i + 1) <
    floor(p 2^32) flips.  Nothing is read back from the device."""

    def __init__(self, cfg, is_train=True):
        inp, aug = cfg.INPUT, getattr(cfg, "AUGMENT", None)
        if is_train:
            mult = tuple(getattr(aug, "MULT_MIN_SIZE_TRAIN", ()))
            min_size = mult if len(mult) > 0 else inp.MIN_SIZE_TRAIN
            max_size = inp.MAX_SIZE_TRAIN
            flip_prob = float(getattr(aug, "FLIP_PROB_TRAIN", 0.5))
            _need(float(getattr(aug, "VERTICAL_FLIP_PROB_TRAIN", 0.0)) == 0.0, "AUGMENT.VERTICAL_FLIP_PROB_TRAIN",
                  "the vertical flip is not built (no FIBER yaml sets it)")
        else:
            min_size, max_size, flip_prob = inp.MIN_SIZE_TEST, inp.MAX_SIZE_TEST, 0.0
        _need(not getattr(inp, "FIX_RES", False), "INPUT.FIX_RES", "the fixed (size, max_size) resolution of Resize(restrict=True) is not built")
        self.min_size = tuple(int(v) for v in (min_size if isinstance(min_size, (list, tuple)) else (min_size,)))
        self.max_size = None if max_size is None else int(max_size)
        self.flip_threshold = int(flip_prob * 2 ** 32)
        self._pixels(cfg)
        self.is_train = bool(is_train)

    def _pixels(self, cfg):
        """the pixel format, mean / std and divisibility: what apply() reads"""
        inp = cfg.INPUT
        fmt = getattr(inp, "FORMAT", "")
        if fmt == "":
            if not getattr(inp, "TO_BGR255", False):
                raise ValueError("INPUT.FORMAT is empty and INPUT.TO_BGR255 is false: build_transforms defines no input format")
            fmt = "bgr255"
        fmt = fmt.lower()
        self.bgr, self.times255 = int("bgr" in fmt), int("255" in fmt)
        self.mean = (lib.C.c_float * 3)(*inp.PIXEL_MEAN)
        self.std = (lib.C.c_float * 3)(*inp.PIXEL_STD)
        self.size_divisible = int(getattr(getattr(cfg, "DATALOADER", None), "SIZE_DIVISIBILITY", 0))

    @classmethod
    def for_views(cls, cfg):
        """A transform for sizes and flips chosen by the caller (multi-scale testing: box_aug.py:73-126 builds Resize(scale, max_size)
        [+ RandomHorizontalFlip(1.0)] + ToTensor + Normalize per view): it carries INPUT's pixel format, mean / std and
        DATALOADER.SIZE_DIVISIBILITY only; apply(images, sizes, flips) is the one call it serves (no size list, no flip probability)."""
        t = cls.__new__(cls)
        t.min_size, t.max_size, t.flip_threshold, t.is_train = (), None, 0, False
        t._pixels(cfg)
        return t

    def choose(self, seed, index, w, h):
        """-> ((oh, ow), flipped) of sample `index` of the batch keyed `seed` for a w x h source"""
        size = self.min_size[hash_u32(seed, 2 * index) % len(self.min_size)]
        return det_resize_size(w, h, size, self.max_size), hash_u32(seed, 2 * index + 1) < self.flip_threshold

    def plan(self, shapes, seed):
        """shapes: (H, W) per image -> (image_sizes, flips, (Hp, Wp)): everything the batch shape depends on, host only."""
        picks = [self.choose(seed, i, W, H) for i, (H, W) in enumerate(shapes)]
        sizes, flips = [p[0] for p in picks], [bool(p[1]) for p in picks]
        return sizes, flips, self.padded_shape(sizes)

    def padded_shape(self, sizes):
        """(Hp, Wp) of to_image_list: the batch maximum, rounded up to DATALOADER.SIZE_DIVISIBILITY (image_list.py:48-60)"""
        Hp, Wp = max(s[0] for s in sizes), max(s[1] for s in sizes)
        if self.size_divisible > 0:
            st = self.size_divisible
            Hp, Wp = (Hp + st - 1) // st * st, (Wp + st - 1) // st * st
        return Hp, Wp

    def __call__(self, images, seed=None):
        if seed is None:
            seed = ops.collate_seed()
        sizes, flips, _ = self.plan([(int(im.shape[0]), int(im.shape[1])) for im in images], int(seed) & _M64)
        return self.apply(images, sizes, flips)

    def apply(self, images, sizes, flips):
        """The device work for choices already made: image i -> sizes[i] = (oh, ow), flipped when flips[i]."""
        n, dev = len(images), images[0].device
        for im in images:
            if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or im.stride(2) != 1 or im.stride(1) != 3:
                raise ValueError("DeviceDetectionTransform needs uint8 [H, W, 3] images with packed pixels")
        shapes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
        sizes, flips = [(int(oh), int(ow)) for oh, ow in sizes], [bool(f) for f in flips]
        Hp, Wp = self.padded_shape(sizes)
        desc = np.zeros(n, _DET_DESC)
        tmp_off = coef_off = 0
        for i, (im, (H, W), (oh, ow)) in enumerate(zip(images, shapes, sizes)):
            if oh < 1 or ow < 1:
                raise ValueError(f"DeviceDetectionTransform: a {H} x {W} image resizes to {oh} x {ow}")
            kh, kv = lib.plain("fiber_resample_ksize_bilinear", W, ow), lib.plain("fiber_resample_ksize_bilinear", H, oh)
            pitch = (3 * ow + 3) // 4 * 4                              # rows of the intermediate start on a dword
            desc[i] = (lib.ptr(im), H, W, int(im.stride(0)), oh, ow, kh, kv, tmp_off, coef_off, coef_off + ow * (2 + kh), int(flips[i]), pitch)
            tmp_off += (H * pitch + 15) // 16 * 16
            coef_off += ow * (2 + kh) + oh * (2 + kv)
        if tmp_off >= 2 ** 31 or coef_off >= 2 ** 31:
            raise ValueError("batch too large for one call (intermediate images exceed 2 GiB): split it")
        d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev, non_blocking=True)
        coef = torch.empty(coef_off, dtype=torch.int32, device=dev)
        tmp = torch.empty(tmp_off + 16, dtype=torch.uint8, device=dev)      # + the slack the dword reads of pass 2 may touch
        out = torch.empty((n, 3, Hp, Wp), dtype=torch.float32, device=dev)
        lib.call("fiber_det_resize_norm_pad_u8", lib.ptr(d_desc), n, lib.ptr(coef), lib.ptr(tmp), lib.ptr(out), Hp, Wp,
                 int(desc["H"].max()), int(desc["oh"].max()), int(desc["ow"].max()), self.bgr, self.times255, self.mean, self.std)
        self._keep = (images, d_desc)          # the sources / table must outlive the (asynchronous) kernels of this call
        return DetImageList(out, sizes, [(H, W, f) for (H, W), f in zip(shapes, flips)])


def pad_input_ids(input_ids, max_query_len, pad_max, pad_id=1):
    """The padding of `batch_encode_plus(padding="max_length" if PAD_MAX else "longest", truncation=True)` (generalized_vl_rcnn.py:268-275)
    on already tokenised ids: a list of 1-D int64 tensors -> {"input_ids", "attention_mask"} int64 [B, L] on the ids' device, the
    mask derived from the ids (1 where id != <pad>)."""
    ids = [torch.as_tensor(t).reshape(-1)[:max_query_len] for t in input_ids]
    L = int(max_query_len) if pad_max else max(int(t.numel()) for t in ids)
    out = torch.full((len(ids), L), pad_id, dtype=torch.int64, device=ids[0].device)
    for i, t in enumerate(ids):
        out[i, :t.numel()] = t
    return {"input_ids": out, "attention_mask": (out != pad_id).long()}


def device_collate_grounding(samples, transform, cfg, seed=None, pad_id=1):
    """The device-side half of the fine-grained loader (data/transforms/build.py, structures/bounding_box.py:101-171,
    structures/image_list.py:30-72, data/collate_batch.py:18-46) for RAW samples.  Each sample is a dict with `image` (uint8 [H, W, 3]
    RGB device tensor), `boxes` ([G, 4] xyxy in the ORIGINAL frame, already clipped by the dataset), `labels` [G], `positive_map`
    [G, 256] and `input_ids` (1-D int64, tokenised with <s> ... </s>).  -> (images: DetImageList, targets: GroundingTargets in the
    resized, flipped frame, tokenizer_input), which GeneralizedVLRCNN.forward(images, targets, tokenizer_input=...) takes as they are.

    JPEG decoding, tokenisation and `create_positive_map` (data/datasets/modulated_coco.py) stay on the host loader and are out of
    scope here: the workers hand over raw bytes, boxes, token ids and the positive map; resizing, flipping, normalising and padding
    the ~12.8 MB of fp32 per 800 x 1333 sample is stream-ordered device work."""
    from .modules.grounding_train import T, pack_targets
    dev = samples[0]["image"].device
    if seed is None:
        seed = ops.collate_seed()
    images = transform([s["image"] for s in samples], seed)
    lb = cfg.MODEL.LANGUAGE_BACKBONE
    tok = pad_input_ids([s["input_ids"] for s in samples], lb.MAX_QUERY_LEN, lb.PAD_MAX, pad_id)
    tok = {k: v.to(dev) for k, v in tok.items()}
    boxes = [torch.as_tensor(s["boxes"]).reshape(-1, 4) for s in samples]
    rows = torch.cat([torch.as_tensor(s["positive_map"]).reshape(b.shape[0], T).cpu() for s, b in zip(samples, boxes)], dim=0)
    targets = pack_targets(boxes, [torch.as_tensor(s["labels"]).reshape(-1) for s in samples], rows, device=dev)
    table = _box_table(images.box_params([int(b.shape[0]) for b in boxes]), dev)
    lib.call("fiber_det_boxes_f32", lib.ptr(targets.boxes), lib.ptr(table), len(samples), int(targets.boxes.shape[1]))
    images._keep = table
    return images, targets, tok


# ---- the coarse-grained model's TRAINING transform -----------------------------------------------------------------------------------
RANDAUG_OPS = ("Identity", "AutoContrast", "Equalize", "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate")
RANDAUG_SKIPPED = -1                                                     # op code of a slot whose coin said "do not apply"
_RANDAUG_UNBUILT = ("Solarize", "Color", "Contrast", "Posterize")        # in randaug.py's func_dict, in no training transform
_RA_SLOT = np.dtype([("op", "<i4"), ("src", "<i4"), ("factor", "<f4"), ("pad", "<i4"), ("m", "<f8", (6,))])
assert _RA_SLOT.itemsize == 64
_RA_CROP_ATTEMPTS = 10


def randaug_forward_matrix(op, arg, size):
    """The 2 x 3 matrix the reference hands to cv2.warpAffine for geometric op `op` (a name of RANDAUG_OPS) with signed argument `arg` on a
    size x size image, as six doubles: shear_x_func / shear_y_func / translate_x_func / translate_y_func build it with np.float32 (the
    entries are float32 widened), rotate_func takes cv2.getRotationMatrix2D((W / 2, H / 2), degree, 1), which is fp64."""
    f = float(np.float32(arg))
    if op == "ShearX":
        return (1.0, f, 0.0, 0.0, 1.0, 0.0)
    if op == "ShearY":
        return (1.0, 0.0, 0.0, f, 1.0, 0.0)
    if op == "TranslateX":
        return (1.0, 0.0, -f, 0.0, 1.0, 0.0)
    if op == "TranslateY":
        return (1.0, 0.0, 0.0, 0.0, 1.0, -f)
    if op != "Rotate":
        raise ValueError(f"{op} is not a geometric op")
    angle = float(arg) * (math.pi / 180.0)
    a, b = math.cos(angle), math.sin(angle)
    cx = cy = float(np.float32(size / 2))
    return (a, b, (1 - a) * cx - b * cy, -b, a, b * cx + (1 - a) * cy)


def warp_affine_inverse(M):
    """cv2.warpAffine's inversion of a forward 2 x 3 matrix (no WARP_INVERSE_MAP), in its order of fp64 operations -> (M0 .. M5), dst -> src."""
    M0, M1, M2, M3, M4, M5 = (float(v) for v in M)
    D = M0 * M4 - M1 * M3
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M4 * D, M0 * D
    M0 = A11
    M1 *= -D
    M3 *= -D
    M4 = A22
    b1 = -M0 * M2 - M1 * M5
    b2 = -M3 * M2 - M4 * M5
    return (M0, M1, b1, M3, M4, b2)


def bilinear_weight_table():
    """cv2's INTER_LINEAR remap weights: int16 [1024, 4], row fy * 32 + fx, column ky * 2 + kx.  The four fp32 products wy[ky] * wx[kx], w =
    (1 - f / 32, f / 32), times 2^15 rounded half-even to a saturating int16 (1 * 1 -> 32767); what the four lack of 2^15 goes to the
    [1][1] tap."""
    f = np.arange(32, dtype=np.float32) * np.float32(1.0 / 32)
    w = np.stack([np.float32(1.0) - f, f], 1)                             # [32, 2]
    tab = (w[:, None, :, None] * w[None, :, None, :]).astype(np.float32)  # [fy, fx, ky, kx]
    it = np.clip(np.rint(tab * np.float32(32768.0)), -32768, 32767).astype(np.int32)
    it[:, :, 1, 1] += 32768 - it.sum((2, 3))
    assert it.min() >= 0 and it.max() <= 32767 and (it.sum((2, 3)) == 32768).all()
    return np.ascontiguousarray(it.reshape(1024, 4).astype(np.int16))


class DeviceRandAugTransform:
    """`albef_transform_randaug(size)` of coarse_grained/fiber/transforms/transform.py:20-45 on the device: RandomResizedCrop(size, scale,
    BICUBIC) -> RandomHorizontalFlip -> RandomAugment(N, M, augs) (transforms/randaug.py) -> ToTensor -> Normalize.  images: list of uint8
    [H, W, 3] RGB device tensors (ragged, row-strided views allowed) -> fp32 [B, 3, size, size].

    `plan(shapes, seed)` draws everything on the host, `apply(images, plan)` is the device work; nothing is read back from the device.
    Draw k of sample i of the batch keyed `seed` is hash_u32(seed, i * (41 + 3 N) + k) / 2^32: k = 4 a .. 4 a + 3 the area, log-ratio, top
    and left of crop attempt a < 10; k = 40 the flip; k = 41 + 3 s .. + 2 slot s's op, its apply coin and its sign.  These streams are NOT
    the reference's (np.random / torch.rand in each loader worker); the distributions are: torchvision's RandomResizedCrop.get_params
    (10 attempts, then the ratio-clamped centre crop), ops uniform with replacement from `augs`, each applied with probability 0.5,
    shear / translate negated when the draw is > 0.5 (randaug.py:212-229), rotate when it is < 0.5 (:260-267).

    What is bit-exact to what: crop + resize + flip equal PIL's `crop(box).resize((size, size), BICUBIC)` / `transpose(FLIP_LEFT_RIGHT)`;
    AutoContrast and Equalize equal PIL.ImageOps (as randaug.py's docstrings promise: the tables are built with `offset = -lo * scale` on
    integers widened to fp64); Brightness and Sharpness restate randaug.py's fp32 arithmetic, Sharpness INCLUDING the wrap of its
    `.astype(np.uint8)` (no clamp: a value below 0 or above 255 keeps its low 8 bits); ShearX / ShearY / TranslateX / TranslateY / Rotate
    follow the arithmetic of OpenCV's generic warpAffine / remap path for 8-bit 3-channel INTER_LINEAR with constant border (128, 128, 128)
    (1/1024 fixed-point coordinates reduced to 1/32, int16 weights summing to 2^15), restated in tests/randaug_cases.py.  Parity of the five
    geometric ops with a particular cv2 build has not been measured by anyone: cv2 is not a dependency of this project.

    Launches per batch, whatever ops were drawn: 1 H2D copy of the plan tables and 3 + 2 max(N, 1) kernels through 1 + max(N, 1) ABI calls
    (fiber_crop_resize_flip_u8: coefficient tables, horizontal pass, vertical pass + flip to bytes; fiber_randaug_slot_u8 per slot: the
    slot's statistics / tables, then its apply, the last one fused with ToTensor + Normalize) -- 7 kernels, 3 calls for N = 2.  The int16
    weight table is uploaded once per transform and device."""

    def __init__(self, size=384, scale=(0.5, 1.0), ratio=(3 / 4, 4 / 3), flip_prob=0.5, N=2, M=7, augs=RANDAUG_OPS, mean=IMAGENET_MEAN,
                 std=IMAGENET_STD):
        self.size, self.N, self.M = int(size), int(N), M
        self.scale, self.ratio = (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1]))
        self.log_ratio = (math.log(self.ratio[0]), math.log(self.ratio[1]))
        self.flip_threshold = int(float(flip_prob) * 2 ** 32)
        for a in augs:
            if a in _RANDAUG_UNBUILT:
                raise NotImplementedError(f"{a}: this RandomAugment op is not built (no training transform of the reference uses it)")
            if a not in RANDAUG_OPS:
                raise ValueError(f"{a}: not an op of transforms/randaug.py")
        if len(augs) < 1 or self.N < 0 or self.size < 1:
            raise ValueError("DeviceRandAugTransform needs at least one op, N >= 0 and size >= 1")
        self.augs = tuple(augs)
        self.codes = tuple(RANDAUG_OPS.index(a) for a in self.augs)
        self.mean = (lib.C.c_float * 3)(*mean)
        self.std = (lib.C.c_float * 3)(*std)
        self.draws = 4 * _RA_CROP_ATTEMPTS + 1 + 3 * self.N
        self.plan_dtype = np.dtype([("top", "<i4"), ("left", "<i4"), ("h", "<i4"), ("w", "<i4"), ("flip", "<i4"),
                                    ("op", "<i4", (self.N,)), ("arg", "<f8", (self.N,))])
        self._wtab = {}

    def level_arg(self, op, negate):
        """randaug.py's arg_dict[op](M) (MAX_LEVEL = 10, translate_const = 10) with the sign draw already made"""
        level = self.M / 10
        if op in ("Brightness", "Sharpness"):
            return level * 1.8 + 0.1
        if op in ("ShearX", "ShearY"):
            level = level * 0.3
        elif op in ("TranslateX", "TranslateY"):
            level = level * float(10)
        elif op == "Rotate":
            level = level * 30
        else:
            return 0.0
        return -level if negate else level

    def crop_box(self, seed, index, H, W):
        """torchvision RandomResizedCrop.get_params for sample `index` -> (top, left, h, w)"""
        base = index * self.draws
        area = H * W
        for a in range(_RA_CROP_ATTEMPTS):
            u = [hash_u32(seed, base + 4 * a + k) / 2.0 ** 32 for k in range(4)]
            target = area * (self.scale[0] + (self.scale[1] - self.scale[0]) * u[0])
            aspect = math.exp(self.log_ratio[0] + (self.log_ratio[1] - self.log_ratio[0]) * u[1])
            w = int(round(math.sqrt(target * aspect)))
            h = int(round(math.sqrt(target / aspect)))
            if 0 < w <= W and 0 < h <= H:
                return int(u[2] * (H - h + 1)), int(u[3] * (W - w + 1)), h, w
        in_ratio = float(W) / float(H)
        if in_ratio < min(self.ratio):
            w = W
            h = int(round(w / min(self.ratio)))
        elif in_ratio > max(self.ratio):
            h = H
            w = int(round(h * max(self.ratio)))
        else:
            w, h = W, H
        return (H - h) // 2, (W - w) // 2, h, w

    def plan(self, shapes, seed):
        """shapes: (H, W) per image -> a numpy record array, one row per image: the crop box `top, left, h, w`, `flip`, and per slot `op`
        (index into RANDAUG_OPS, RANDAUG_SKIPPED when the slot's coin said no) and `arg` (the signed magnitude of a geometric op, the factor
        of Brightness / Sharpness, else 0).  A pure function of (shapes, seed)."""
        seed = int(seed) & _M64
        p = np.zeros(len(shapes), self.plan_dtype)
        for i, (H, W) in enumerate(shapes):
            H, W = int(H), int(W)
            base = i * self.draws + 4 * _RA_CROP_ATTEMPTS
            p[i]["top"], p[i]["left"], p[i]["h"], p[i]["w"] = self.crop_box(seed, i, H, W)
            p[i]["flip"] = int(hash_u32(seed, base) < self.flip_threshold)
            for s in range(self.N):
                pick, coin, sign = (hash_u32(seed, base + 1 + 3 * s + k) for k in range(3))
                name = self.augs[(pick * len(self.augs)) >> 32]
                if coin >= 2 ** 31:                                          # `if np.random.random() > prob: continue`
                    p[i]["op"][s] = RANDAUG_SKIPPED
                    continue
                negate = sign < 2 ** 31 if name == "Rotate" else sign >= 2 ** 31
                p[i]["op"][s] = RANDAUG_OPS.index(name)
                p[i]["arg"][s] = self.level_arg(name, negate)
        return p

    def __call__(self, images, seed=None):
        if seed is None:
            seed = ops.collate_seed()
        return self.apply(images, self.plan([(int(im.shape[0]), int(im.shape[1])) for im in images], seed))

    def apply(self, images, plan, return_u8=False):
        """The device work for a plan (of `plan`, or hand-written with `plan_dtype`): -> fp32 [B, 3, size, size]; with return_u8 also the
        uint8 [B, size, size, 3] image as it stood just before ToTensor."""
        S, n, dev = self.size, len(images), images[0].device
        K = max(self.N, 1)
        if len(plan) != n or plan.dtype != self.plan_dtype:
            raise ValueError(f"DeviceRandAugTransform.apply: a plan of {len(plan)} rows ({plan.dtype}) for {n} images")
        desc, slots = np.zeros(n, _DESC), np.zeros((K, n), _RA_SLOT)
        slots["op"] = RANDAUG_SKIPPED
        tmp_off = coef_off = 0
        for i, (im, p) in enumerate(zip(images, plan)):
            if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or im.stride(2) != 1 or im.stride(1) != 3:
                raise ValueError("DeviceRandAugTransform needs uint8 [H, W, 3] images with packed pixels")
            H, W = int(im.shape[0]), int(im.shape[1])
            top, left, h, w = int(p["top"]), int(p["left"]), int(p["h"]), int(p["w"])
            if not (0 <= top and 0 <= left and 0 < h and 0 < w and top + h <= H and left + w <= W):
                raise ValueError(f"DeviceRandAugTransform.apply: crop box {(top, left, h, w)} outside image {i} ({H} x {W})")
            stride = int(im.stride(0))
            kh, kv = lib.plain("fiber_resample_ksize", w, S), lib.plain("fiber_resample_ksize", h, S)
            desc[i] = (lib.ptr(im) + top * stride + left * 3, h, w, stride, kh, kv, tmp_off, coef_off, coef_off + S * (2 + kh))
            tmp_off += (h * S * 3 + 15) // 16 * 16
            coef_off += S * (2 + kh) + S * (2 + kv)
            cur = 0                                                          # which byte image holds the sample: the ping-pong
            for s in range(K):
                sl = slots[s, i]
                sl["src"] = cur                                              # a skipped LAST slot still reads the sample to normalise it
                op = int(p["op"][s]) if s < self.N else RANDAUG_SKIPPED
                if op < 0:
                    continue
                if op >= len(RANDAUG_OPS):
                    raise ValueError(f"DeviceRandAugTransform.apply: op code {op} in slot {s} of image {i}")
                sl["op"] = op
                name = RANDAUG_OPS[op]
                if name in ("Brightness", "Sharpness"):
                    sl["factor"] = p["arg"][s]
                elif op >= RANDAUG_OPS.index("ShearX"):
                    sl["m"] = warp_affine_inverse(randaug_forward_matrix(name, float(p["arg"][s]), S))
                if op >= RANDAUG_OPS.index("Sharpness") and s < K - 1:
                    cur ^= 1                                                 # Sharpness and the gather write the other image
        if tmp_off >= 2 ** 31 or coef_off >= 2 ** 31:
            raise ValueError("batch too large for one call (intermediate images exceed 2 GiB): split it")
        pitch = (S * S * 3 + 15) // 16 * 16
        blob = np.concatenate([slots.reshape(-1).view(np.uint8), desc.view(np.uint8), plan["flip"].astype("<i4").view(np.uint8)])
        d_blob = torch.from_numpy(blob).to(dev, non_blocking=True)
        p_slots = lib.ptr(d_blob)
        p_desc = p_slots + K * n * 64
        p_flip = p_desc + n * 40
        key = (dev.type, dev.index)
        if key not in self._wtab:
            self._wtab[key] = torch.from_numpy(bilinear_weight_table()).to(dev)
        wtab = self._wtab[key]
        coef = torch.empty(coef_off, dtype=torch.int32, device=dev)
        tmp = torch.empty(tmp_off, dtype=torch.uint8, device=dev)
        bufs = torch.empty(2 * n * pitch, dtype=torch.uint8, device=dev)
        luts = torch.empty(n * 768, dtype=torch.uint8, device=dev)
        out = torch.empty((n, 3, S, S), dtype=torch.float32, device=dev)
        u8 = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev) if return_u8 else None
        b0 = lib.ptr(bufs)
        b1 = b0 + n * pitch
        lib.call("fiber_crop_resize_flip_u8", p_desc, p_flip, n, lib.ptr(coef), lib.ptr(tmp), b0, pitch, S, int(desc["H"].max()))
        for s in range(K):
            last = s == K - 1
            lib.call("fiber_randaug_slot_u8", p_slots + s * n * 64, n, b0, b1, pitch, lib.ptr(luts), lib.ptr(wtab), S,
                     lib.ptr(out) if last else None, lib.ptr(u8) if last else None, self.mean, self.std)
        self._keep = (images, d_blob)          # the sources / tables must outlive the (asynchronous) kernels of this call
        return (out, u8) if return_u8 else out


def keys_to_transforms(keys, size=384):
    """coarse_grained/fiber/transforms/__init__.py:12 for the device transforms: config["train_transform_keys"] / ["val_transform_keys"] ->
    a list of transforms for `device_collate`."""
    table = {"albef": DeviceImageTransform, "albef_randaug": DeviceRandAugTransform}
    for k in keys:
        if k not in table:
            raise KeyError(f"{k}: no device transform of that name (known: {sorted(table)})")
    return [table[k](size=size) for k in keys]
