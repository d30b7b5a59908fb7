"""Case table and numpy restatements of the fine-grained (grounding) model's input pipeline (fiber_amd/data.py DeviceDetectionTransform /
device_collate_grounding, csrc/input.hip det_* kernels).  Shared by tests/test_det_input_host.py (the restatements against PIL, the
PIL-produced fixtures tests/golden/det_resize_*.npz and the reference-run fixture tests/golden/det_boxes.npz), tests/test_hip_det_input.py
(the kernels against the restatements, bit for bit) and tools/gen_det_input_golden.py.  Nothing here needs a GPU or PIL to import.

The reference chain (fine_grained/maskrcnn_benchmark): data/transforms/build.py `build_transforms` = Resize(min, max) -> RandomHorizontalFlip ->
ToTensor -> Normalize(format); structures/bounding_box.py `BoxList.resize` / `transpose(0)`; structures/image_list.py `to_image_list(32)`.
  resize     PIL Image.resize((ow, oh), BILINEAR) = Pillow ImagingResample with the triangle filter 1 - |x|, support 1 x max(scale, 1):
             windows normalised in double, quantised to 22 bits, 8-bit rounding after each pass, horizontal first, an unchanged axis skipped
  flip       columns reversed (F.hflip)
  to-tensor  fp32 v / 255, CHW
  normalise  channels [2, 1, 0] if "bgr" in format; x 255 if "255" in format; (x - mean[c]) / std[c], c the channel AFTER the swap
  pad        zeros up to the batch maximum rounded up to the divisibility, after normalising
Everything is integer arithmetic or single correctly rounded fp32 operations, so the device result is compared with np.array_equal."""
import numpy as np

from oracle.image_ref import PRECISION_BITS, hash_u32

# name: (H, W, oh, ow) -- the six shapes on which the restatement was first found bit-equal to PIL: down, up, mixed, identity, the
# max_size cap (61 x 200 at size 40 / max 90) and an odd up-scale
RESIZE_CASES = {
    "det_resize_down": (97, 131, 64, 86),
    "det_resize_up": (20, 30, 43, 64),
    "det_resize_mixed": (150, 40, 97, 26),
    "det_resize_same": (64, 64, 64, 64),
    "det_resize_cap": (61, 200, 27, 88),
    "det_resize_up_odd": (33, 47, 80, 113),
}
BGR255_MEAN, BGR255_STD = (103.530, 116.280, 123.675), (57.375, 57.120, 58.395)      # the FIBER yamls' INPUT.PIXEL_MEAN / PIXEL_STD
RGB_MEAN, RGB_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

# (w, h, size, max_size) -> (oh, ow): Resize.get_size (transforms.py:94-116) worked by hand
SIZE_TABLE = [
    ((200, 61, 40, 90), (27, 88)),        # the cap engaged: 200 / 61 * 40 = 131.1 > 90 -> size = round(90 * 61 / 200) = 27; ow = int(27 * 200 / 61) = 88
    ((131, 97, 64, 133), (64, 86)),       # landscape: oh = size, ow = int(64 * 131 / 97) = 86
    ((40, 150, 64, 133), (131, 35)),      # portrait, capped: 150 / 40 * 64 = 240 > 133 -> size = round(133 * 40 / 150) = 35; oh = int(35 * 150 / 40) = 131
    ((64, 64, 64, 133), (64, 64)),        # square, the early return
    ((100, 64, 64, 133), (64, 100)),      # the early return keeps (h, w): the short side already equals size
    ((64, 100, 64, 133), (100, 64)),      # ... portrait
    ((30, 20, 48, 133), (48, 72)),        # an upscale: ow = int(48 * 30 / 20) = 72
    ((47, 33, 80, 133), (80, 113)),       # an upscale, odd sizes: int(80 * 47 / 33) = int(113.9) = 113
    ((200, 2, 48, 133), (1, 100)),        # a sliver: size = round(133 * 2 / 200) = 1; ow = int(1 * 200 / 2) = 100
    ((50, 80, 64, None), (102, 64)),      # no max_size: oh = int(64 * 80 / 50) = 102
    ((640, 480, 800, 1333), (800, 1066)),  # the flagship size: int(800 * 640 / 480) = 1066
]


def synth_image(H, W, seed):
    """A small uint8 [H, W, 3] image with structure: gradients, noise and saturated patches"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([(xx * 255 // max(1, W - 1)), (yy * 255 // max(1, H - 1)), ((xx + yy) % 256)], -1).astype(np.int64)
    img = img + g.integers(-40, 41, (H, W, 3))
    img[: H // 5, : W // 4] = 255
    img[H - H // 6:, W - W // 3:] = 0
    return np.clip(img, 0, 255).astype(np.uint8)


def case_image(name):
    H, W = RESIZE_CASES[name][:2]
    return synth_image(H, W, seed=H * 1000 + W)


# ---- Pillow's resampler with the triangle filter -------------------------------------------------------------------------------------
def _triangle(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def precompute_coeffs_bilinear(in_size, out_size):
    """Pillow precompute_coeffs + normalize_coeffs_8bpc with bilinear_filter (support 1.0): (bounds [out, 2], coefficients [out, ksize])."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int64)
    kk = np.zeros((out_size, ksize), np.int64)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_triangle((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _pass(img, out_size, axis):
    in_size = img.shape[axis]
    if in_size == out_size:
        return img                                          # ImagingResample: need_horizontal / need_vertical false
    bounds, kk = precompute_coeffs_bilinear(in_size, out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    for xx in range(out_size):
        xmin, xmax = bounds[xx]
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(kk[xx, :xmax], src[xmin:xmin + xmax], axes=(0, 0))
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_bilinear_u8(img, oh, ow):
    """PIL `Image.resize((ow, oh), Image.BILINEAR)` of a uint8 [H, W, 3] array: horizontal pass, then vertical."""
    return _pass(_pass(np.ascontiguousarray(img), ow, 1), oh, 0)


# ---- the transform chain and the batch --------------------------------------------------------------------------------------------------
def normalize_ref(resized, flip, fmt, mean, std):
    """uint8 [oh, ow, 3] -> fp32 [3, oh, ow]: hflip -> ToTensor -> Normalize(format), each operation rounded to fp32"""
    r = resized[:, ::-1] if flip else resized
    t = np.transpose(r.astype(np.float32) / np.float32(255.0), (2, 0, 1))
    if "bgr" in fmt:
        t = t[[2, 1, 0]]
    if "255" in fmt:
        t = t * np.float32(255.0)
    m = np.asarray(mean, np.float32)[:, None, None]
    s = np.asarray(std, np.float32)[:, None, None]
    return ((t - m) / s).astype(np.float32)


def get_size_ref(w, h, size, max_size):
    """Resize.get_size, written independently of fiber_amd.data.det_resize_size (integer / float steps spelled out)"""
    if max_size is not None:
        lo, hi = float(min(w, h)), float(max(w, h))
        if hi / lo * size > max_size:
            size = int(round(max_size * lo / hi))
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    return (int(size * h / w), size) if w < h else (size, int(size * w / h))


def choices_ref(seed, shapes, min_sizes, max_size, flip_prob):
    """-> [((oh, ow), flip)] of a batch of (H, W) shapes: draw 2i picks the size, draw 2i + 1 flips below floor(p 2^32)"""
    out = []
    for i, (H, W) in enumerate(shapes):
        size = min_sizes[hash_u32(seed, 2 * i) % len(min_sizes)]
        out.append((get_size_ref(W, H, size, max_size), hash_u32(seed, 2 * i + 1) < int(flip_prob * 2 ** 32)))
    return out


def batch_ref(images, choices, fmt, mean, std, divisible):
    """-> fp32 [B, 3, Hp, Wp]: every image through the chain, zero-padded as to_image_list pads"""
    per = [normalize_ref(resize_bilinear_u8(im, oh, ow), flip, fmt, mean, std) for im, ((oh, ow), flip) in zip(images, choices)]
    Hp, Wp = max(p.shape[1] for p in per), max(p.shape[2] for p in per)
    if divisible > 0:
        Hp, Wp = -(-Hp // divisible) * divisible, -(-Wp // divisible) * divisible
    out = np.zeros((len(per), 3, Hp, Wp), np.float32)
    for b, p in enumerate(per):
        out[b, :, :p.shape[1], :p.shape[2]] = p
    return out


# ---- boxes ------------------------------------------------------------------------------------------------------------------------------
# name: ((orig_w, orig_h), (new_w, new_h), flip) -- equal ratios (the reference's single-ratio branch), unequal ratios, a flip at odd
# width, an up-scale with a flip, the identity
BOX_CASES = {
    "equal": ((100, 50), (200, 100), False),
    "unequal": ((131, 97), (86, 64), False),
    "flip_odd": ((131, 97), (87, 64), True),
    "up_flip": ((47, 33), (113, 80), True),
    "same_flip": ((64, 64), (64, 64), True),
}
BOX_GOLDEN = "det_boxes"


def case_boxes(name, n=7):
    """Seeded xyxy boxes inside the original frame (fp32, fractional), as a dataset leaves them after clipping"""
    (w, h), _, _ = BOX_CASES[name]
    g = np.random.default_rng(sum(map(ord, name)))
    x = np.sort(g.uniform(0, w - 1, (n, 2)), axis=1)
    y = np.sort(g.uniform(0, h - 1, (n, 2)), axis=1)
    b = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1).astype(np.float32)
    b[0] = (0.0, 0.0, w - 1, h - 1)                               # the whole frame
    return b


def boxes_ref(boxes, orig_wh, new_wh, flip):
    """BoxList.resize((new_w, new_h)) then, when flip, BoxList.transpose(FLIP_LEFT_RIGHT) in fp32: the ratios are formed in double and
    rounded to fp32 (a tensor times a python float), the flip is (new_w - x_max) - 1 and (new_w - x_min) - 1."""
    rw = np.float32(float(new_wh[0]) / float(orig_wh[0]))
    rh = np.float32(float(new_wh[1]) / float(orig_wh[1]))
    b = np.asarray(boxes, np.float32)
    x0, y0, x1, y1 = b[:, 0] * rw, b[:, 1] * rh, b[:, 2] * rw, b[:, 3] * rh
    if flip:
        w = np.float32(new_wh[0])
        x0, x1 = (w - x1) - np.float32(1), (w - x0) - np.float32(1)
    return np.stack([x0, y0, x1, y1], axis=1).astype(np.float32)


# ---- configuration ------------------------------------------------------------------------------------------------------------------------
def input_cfg(cfg=None, min_size=(48, 64, 80), max_size=133, flip=0.5, fmt="", to_bgr255=True, mean=BGR255_MEAN, std=BGR255_STD, divisible=32,
              mult=(), fix_res=False, vflip=0.0, max_query_len=256, pad_max=True):
    """The nodes build_transforms, BatchCollator and the tokenizer call read, attached to `cfg` (default: a bare namespace)"""
    import types
    ns = types.SimpleNamespace
    cfg = cfg if cfg is not None else ns(MODEL=ns(LANGUAGE_BACKBONE=ns(MAX_QUERY_LEN=max_query_len, PAD_MAX=pad_max)))
    cfg.INPUT = ns(MIN_SIZE_TRAIN=min_size, MAX_SIZE_TRAIN=max_size, MIN_SIZE_TEST=min_size[0], MAX_SIZE_TEST=max_size, PIXEL_MEAN=list(mean),
                   PIXEL_STD=list(std), FORMAT=fmt, TO_BGR255=to_bgr255, FIX_RES=fix_res)
    cfg.AUGMENT = ns(MULT_MIN_SIZE_TRAIN=mult, FLIP_PROB_TRAIN=flip, VERTICAL_FLIP_PROB_TRAIN=vflip)
    cfg.DATALOADER = ns(SIZE_DIVISIBILITY=divisible)
    return cfg
