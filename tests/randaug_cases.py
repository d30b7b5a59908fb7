"""The coarse-grained TRAINING transform restated in numpy, stage by stage, and the hand-written plans the GPU test runs.

Reference: coarse_grained/fiber/transforms/transform.py:20-45 `albef_transform_randaug` = RandomResizedCrop(size, scale=(0.5, 1.0), BICUBIC) ->
RandomHorizontalFlip -> RandomAugment(2, 7, isPIL=True, augs=[the ten ops below]) (transforms/randaug.py) -> ToTensor -> Normalize.

  * crop, resize, flip go through PIL itself (torchvision's resized_crop / hflip on a PIL image are `img.crop(box).resize((S, S), BICUBIC)` and
    `transpose(FLIP_LEFT_RIGHT)`);
  * AutoContrast, Equalize, Brightness, Sharpness restate randaug.py line by line, with np.bincount in place of cv2.calcHist and the 3 x 3
    blur as `(2 T + 13) // 26` (T = the 3 x 3 sum + 4 x the centre: cv2.filter2D's rounded output, T / 13 never sits on a half);
  * ShearX / ShearY / TranslateX / TranslateY / Rotate restate the arithmetic of OpenCV's generic warpAffine / remap path for 8-bit, 3-channel,
    INTER_LINEAR, BORDER_CONSTANT (`warp` below).  cv2 is not installed where this project is built and randaug.py cannot be imported without
    it: parity of `warp` with a particular cv2 build has NOT been measured by anyone.  tests/test_randaug_host.py pins it against PIL's affine
    transform instead (exactly for the translations, within the 1/32-pixel quantisation for shear and rotate).

Nothing here imports fiber_amd: the device code and its host half are what these functions judge."""
import math

import numpy as np
from PIL import Image

OPS = ("Identity", "AutoContrast", "Equalize", "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate")
GEOMETRIC = OPS[5:]
SKIP = -1
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
M = 7                                                            # RandomAugment(2, 7): the level of every training config
SHEAR, TRANSLATE, ROTATE, ENHANCE = (M / 10) * 0.3, (M / 10) * float(10), (M / 10) * 30, (M / 10) * 1.8 + 0.1
FILL = 128                                                       # randaug.py replace_value = (128, 128, 128)


# ---- crop, resize, flip ------------------------------------------------------------------------------------------------------------------
def crop_resize_flip(img, box, S, flip):
    top, left, h, w = box
    out = Image.fromarray(img).crop((left, top, left + w, top + h)).resize((S, S), Image.BICUBIC)
    if flip:
        out = out.transpose(Image.FLIP_LEFT_RIGHT)
    return np.array(out)


# ---- the table ops ----------------------------------------------------------------------------------------------------------------------
def autocontrast_table(ch):
    """randaug.py:19-38 with cutoff = 0 (`high`, `low` as integers: offset = -low * scale, the value PIL.ImageOps.autocontrast uses)"""
    high, low = int(ch.max()), int(ch.min())
    if high <= low:
        return np.arange(256).astype(np.uint8)
    scale = 255 / (high - low)
    offset = -low * scale
    table = np.arange(256) * scale + offset
    table[table < 0] = 0
    table[table > 255] = 255
    return table.clip(0, 255).astype(np.uint8)


def equalize_table(ch):
    """randaug.py:53-63"""
    hist = np.bincount(ch.reshape(-1), minlength=256).astype(np.int64)
    non_zero = hist[hist != 0]
    step = int(np.sum(non_zero[:-1])) // 255
    if step == 0:
        return np.arange(256).astype(np.uint8)
    n = np.empty_like(hist)
    n[0] = step // 2
    n[1:] = hist[:-1]
    return (np.cumsum(n) // step).clip(0, 255).astype(np.uint8)


def autocontrast(img):
    return np.stack([autocontrast_table(img[..., c])[img[..., c]] for c in range(3)], -1)


def equalize(img):
    return np.stack([equalize_table(img[..., c])[img[..., c]] for c in range(3)], -1)


def brightness(img, factor):
    table = (np.arange(256, dtype=np.float32) * np.float32(factor)).clip(0, 255).astype(np.uint8)
    return table[img]


# ---- Sharpness ----------------------------------------------------------------------------------------------------------------------------
def blur_interior(img):
    """cv2.filter2D(img, -1, [[1, 1, 1], [1, 5, 1], [1, 1, 1]] / 13) on the interior [1:-1, 1:-1]: int64 [H - 2, W - 2, 3]"""
    a = img.astype(np.int64)
    H, W = a.shape[:2]
    T = 4 * a[1:-1, 1:-1]
    for dy in range(3):
        for dx in range(3):
            T = T + a[dy:H - 2 + dy, dx:W - 2 + dx]
    return (2 * T + 13) // 26


def sharpness_raw(img, factor):
    """randaug.py:142-144 before the cast: fp32 [H, W, 3]"""
    out = img.astype(np.float32)
    if min(img.shape[:2]) >= 3:
        deg = blur_interior(img).astype(np.float32)
        out[1:-1, 1:-1, :] = deg + np.float32(factor) * (out[1:-1, 1:-1, :] - deg)
    return out


def sharpness(img, factor):
    """... and `.astype(np.uint8)`, which WRAPS: truncation toward zero, then the low 8 bits"""
    return sharpness_raw(img, factor).astype(np.int32).astype(np.uint8)


# ---- the affine gather: OpenCV warpAffine, generic path, 8UC3 INTER_LINEAR BORDER_CONSTANT ------------------------------------------------
def forward_matrix(op, arg, H, W):
    """What randaug.py hands to cv2.warpAffine: np.float32 matrices for shear / translate (widened to fp64 by warpAffine),
    cv2.getRotationMatrix2D((W / 2, H / 2), degree, 1) (fp64) for rotate.  -> fp64 [6]"""
    if op == "ShearX":
        m = np.float32([[1, arg, 0], [0, 1, 0]])
    elif op == "ShearY":
        m = np.float32([[1, 0, 0], [arg, 1, 0]])
    elif op == "TranslateX":
        m = np.float32([[1, 0, -arg], [0, 1, 0]])
    elif op == "TranslateY":
        m = np.float32([[1, 0, 0], [0, 1, -arg]])
    else:
        assert op == "Rotate", op
        angle = arg * (math.pi / 180)
        alpha, beta = math.cos(angle), math.sin(angle)
        cx, cy = float(np.float32(W / 2)), float(np.float32(H / 2))
        m = np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], np.float64)
    return m.astype(np.float64).reshape(6)


def invert(m):
    """warpAffine's own inversion (imgwarp.cpp), operation by operation in fp64"""
    m = [float(v) for v in m]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11
    m[1] *= -D
    m[3] *= -D
    m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def weight_table():
    """initInterTab2D(INTER_LINEAR, fixpt): int [32 (fy), 32 (fx), 2 (ky), 2 (kx)]"""
    tab = np.zeros((32, 32, 2, 2), np.int64)
    one = [(np.float32(1.0) - np.float32(i) * np.float32(1.0 / 32), np.float32(i) * np.float32(1.0 / 32)) for i in range(32)]
    for fy in range(32):
        for fx in range(32):
            for ky in range(2):
                for kx in range(2):
                    v = np.float32(one[fy][ky] * one[fx][kx]) * np.float32(32768)
                    tab[fy, fx, ky, kx] = min(32767, max(-32768, int(np.rint(v))))          # saturate_cast<short>
            tab[fy, fx, 1, 1] += 32768 - tab[fy, fx].sum()
    return tab


_WTAB = weight_table()


def source_map(minv, H, W):
    """-> (sx, sy, fx, fy) int64 [H, W]: the top-left tap and the 1/32 fractions of every destination pixel"""
    m0, m1, m2, m3, m4, m5 = minv
    x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    adelta = np.rint(m0 * x * 1024).astype(np.int64)
    bdelta = np.rint(m3 * x * 1024).astype(np.int64)
    X0 = np.rint((m1 * y + m2) * 1024).astype(np.int64) + 16
    Y0 = np.rint((m4 * y + m5) * 1024).astype(np.int64) + 16
    X = (X0[:, None] + adelta[None, :]) >> 5
    Y = (Y0[:, None] + bdelta[None, :]) >> 5
    return X >> 5, Y >> 5, X & 31, Y & 31


def warp(img, minv):
    H, W = img.shape[:2]
    sx, sy, fx, fy = source_map(minv, H, W)
    w = _WTAB[fy, fx]                                              # [H, W, 2, 2]
    a = img.astype(np.int64)
    acc = np.full((H, W, 3), 16384, np.int64)
    for ky in range(2):
        for kx in range(2):
            yy, xx = sy + ky, sx + kx
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            tap = np.where(inside[..., None], a[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], FILL)
            acc += w[:, :, ky, kx, None] * tap
    out = np.clip(acc >> 15, 0, 255)
    outside = (sx >= W) | (sx + 1 < 0) | (sy >= H) | (sy + 1 < 0)
    out[outside] = FILL
    return out.astype(np.uint8)


# ---- one op, one sample -------------------------------------------------------------------------------------------------------------------
def apply_op(img, code, arg):
    if code in (SKIP, 0):
        return img
    name = OPS[code]
    if name == "AutoContrast":
        return autocontrast(img)
    if name == "Equalize":
        return equalize(img)
    if name == "Brightness":
        return brightness(img, arg)
    if name == "Sharpness":
        return sharpness(img, arg)
    return warp(img, invert(forward_matrix(name, arg, img.shape[0], img.shape[1])))


def to_tensor_normalize(u8, mean=MEAN, std=STD):
    t = np.transpose(u8.astype(np.float32) / np.float32(255.0), (2, 0, 1))
    return ((t - np.asarray(mean, np.float32)[:, None, None]) / np.asarray(std, np.float32)[:, None, None]).astype(np.float32)


def sample_ref(img, case, S):
    """case = (box, flip, [(code, arg), ...]) -> (uint8 [S, S, 3] before ToTensor, fp32 [3, S, S])"""
    box, flip, slots = case
    u8 = crop_resize_flip(img, box, S, flip)
    for code, arg in slots:
        u8 = apply_op(u8, code, arg)
    return u8, to_tensor_normalize(u8)


# ---- sources ----------------------------------------------------------------------------------------------------------------------------
SHAPES = ((37, 53), (64, 48), (21, 21))


def synth_image(H, W, seed):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([40 + xx * 170 // max(1, W - 1), 30 + yy * 200 // max(1, H - 1), 20 + (3 * xx + 2 * yy) % 200], -1).astype(np.int64)
    img = img + g.integers(-25, 26, (H, W, 3))
    img[: H // 5, : W // 4] = 250
    img[H - H // 6:, W - W // 3:] = 8
    return np.clip(img, 0, 255).astype(np.uint8)


def source(kind):
    """kind: 0, 1, 2 = a structured image of SHAPES[kind]; "flat" = a constant 21 x 21; "checker" = a 0 / 255 checkerboard of 5-pixel cells,
    64 x 48; "narrow" = 37 x 53 with values in [100, 140]"""
    if kind == "flat":
        return np.full((21, 21, 3), (7, 130, 255), np.uint8)
    if kind == "checker":
        yy, xx = np.mgrid[0:64, 0:48]
        return np.repeat((((yy // 5 + xx // 5) % 2) * 255).astype(np.uint8)[..., None], 3, -1)
    if kind == "narrow":
        return (100 + np.random.default_rng(11).integers(0, 41, (37, 53, 3))).astype(np.uint8)
    H, W = SHAPES[kind]
    return synth_image(H, W, seed=H * 100 + W)


def code(name):
    return OPS.index(name)


def _arg(name, sign):
    if name in ("ShearX", "ShearY"):
        return sign * SHEAR
    if name in ("TranslateX", "TranslateY"):
        return sign * TRANSLATE
    if name == "Rotate":
        return sign * ROTATE
    if name in ("Brightness", "Sharpness"):
        return ENHANCE
    return 0.0


def slot(name, sign=1):
    return (SKIP, 0.0) if name is None else (code(name), _arg(name, sign))


def _box(kind, which, S):
    """crop boxes (top, left, h, w) of a source: the whole image, boxes touching each edge, an inner one, one of the output size"""
    H, W = source(kind).shape[:2]
    h, w = max(2, (3 * H) // 4), max(2, (3 * W) // 4)
    return {"full": (0, 0, H, W), "top": (0, 3, h, w - 3), "left": (2, 0, h - 2, w), "bottom": (H - h, 1, h, w), "right": (1, W - w, h, w),
            "inner": (2, 3, h - 3, w - 4), "same": (1, 2, min(S, H - 1), min(S, W - 2))}[which]


_BOXES = ("full", "top", "left", "bottom", "right", "inner", "same")


def single_slot_cases(position, S):
    """Every op alone in slot `position` (the other slot skipped), both signs of the geometric ones: 15 samples, mixed sources, boxes, flips"""
    names = [(n, 1) for n in OPS[:5]] + [(n, s) for n in GEOMETRIC for s in (1, -1)]
    out = []
    for i, (n, s) in enumerate(names):
        kind = i % 3
        slots = [slot(None), slot(None)]
        slots[position] = slot(n, s)
        out.append((kind, (_box(kind, _BOXES[i % len(_BOXES)], S), i % 2 == 1, slots)))
    return out


def pair_cases(S):
    """Slot 2 after slot 1 (the statistics of slot 2 must see slot 1's OUTPUT, fill pixels included), the identity branches, the wrap"""
    P = [
        (0, "full", False, ("AutoContrast", 1), ("Equalize", 1)),
        (1, "inner", True, ("Sharpness", 1), ("AutoContrast", 1)),
        (2, "full", False, ("Rotate", 1), ("Equalize", 1)),
        (0, "right", True, ("Rotate", -1), ("AutoContrast", 1)),
        (1, "top", False, ("ShearX", 1), ("Rotate", -1)),               # warp after warp
        (2, "left", True, ("TranslateX", -1), ("TranslateY", 1)),
        (0, "bottom", False, ("Sharpness", 1), ("Sharpness", 1)),       # the same op twice
        (1, "full", True, ("Rotate", 1), ("Rotate", 1)),
        (2, "inner", False, ("Equalize", 1), ("Equalize", 1)),
        (0, "same", False, ("Brightness", 1), ("Brightness", 1)),
        ("flat", "full", False, ("AutoContrast", 1), ("Equalize", 1)),  # hi <= lo and step == 0: both tables are the identity
        ("flat", "full", True, ("Equalize", 1), ("ShearY", -1)),
        ("checker", "full", False, ("Sharpness", 1), None),             # wraps below 0 and above 255
        ("checker", "inner", True, None, ("Sharpness", 1)),
        ("narrow", "full", False, ("Equalize", 1), ("AutoContrast", 1)),
        ("narrow", "right", True, ("Identity", 1), ("Sharpness", 1)),
    ]
    return [(kind, (_box(kind, b, S), f, [slot(*(a or (None,))), slot(*(c or (None,)))])) for kind, b, f, a, c in P]


def skipped_cases(S):
    """every slot skipped: crops touching each edge, flip on and off"""
    return [(i % 3, (_box(i % 3, b, S), f, [slot(None), slot(None)])) for i, (b, f) in
            enumerate((b, f) for b in _BOXES for f in (False, True))][:14]


def batch_ref(cases, S):
    """-> (host images, uint8 [B, S, S, 3], fp32 [B, 3, S, S])"""
    imgs = [source(kind) for kind, _ in cases]
    refs = [sample_ref(im, case, S) for im, (_, case) in zip(imgs, cases)]
    return imgs, np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs])
