"""CPU tests of the training transform's host half: the numpy restatement of tests/randaug_cases.py pinned against PIL (what randaug.py's
docstrings promise), and DeviceRandAugTransform.plan's determinism and distributions.  Nothing here needs a GPU."""
import math

import numpy as np
import pytest
from PIL import Image, ImageFilter, ImageOps

import randaug_cases as rc


def _pinning_images():
    """300 small images: structured ones, constant, two-valued, narrow-range and single-outlier ones"""
    g = np.random.default_rng(0)
    out = []
    for i in range(300):
        H, W = int(g.integers(3, 40)), int(g.integers(3, 40))
        k = i % 6
        if k == 0:
            img = np.broadcast_to(g.integers(0, 256, 3), (H, W, 3))
        elif k == 1:
            lo, hi = sorted(g.integers(0, 256, 2))
            img = np.where(g.random((H, W, 3)) < 0.5, lo, hi)
        elif k == 2:
            lo = int(g.integers(0, 250))
            img = lo + g.integers(0, int(g.integers(1, 6)) + 1, (H, W, 3))
        elif k == 3:
            img = rc.synth_image(H, W, i)
        elif k == 4:
            img = np.full((H, W, 3), int(g.integers(0, 256)))
            img[int(g.integers(0, H)), int(g.integers(0, W))] = g.integers(0, 256, 3)
        else:
            img = g.integers(0, 256, (H, W, 3))
        out.append(np.ascontiguousarray(np.clip(img, 0, 255).astype(np.uint8)))
    return out


IMAGES = _pinning_images()


def test_autocontrast_and_equalize_equal_pil():
    for i, img in enumerate(IMAGES):
        pil = Image.fromarray(img)
        assert np.array_equal(rc.autocontrast(img), np.array(ImageOps.autocontrast(pil))), i
        assert np.array_equal(rc.equalize(img), np.array(ImageOps.equalize(pil))), i


def test_sharpness_blur_equals_pil_smooth_on_the_interior():
    for i, img in enumerate(IMAGES[:120]):
        smooth = np.array(Image.fromarray(img).filter(ImageFilter.SMOOTH))
        assert np.array_equal(rc.blur_interior(img), smooth[1:-1, 1:-1]), i
    # the border ring keeps the input, and the cast wraps instead of clamping
    img = rc.crop_resize_flip(rc.source("checker"), (0, 0, 64, 48), 30, False)
    raw, out = rc.sharpness_raw(img, rc.ENHANCE), rc.sharpness(img, rc.ENHANCE)
    assert raw.min() <= -1 and raw.max() >= 256
    assert np.array_equal(out[0], img[0]) and np.array_equal(out[-1], img[-1]) and np.array_equal(out[:, 0], img[:, 0])
    assert np.array_equal(out[:, -1], img[:, -1])
    assert np.array_equal(out, np.trunc(raw).astype(np.int64) & 255)
    assert (out[raw <= -1] > 128).all() and (out[raw >= 256] < 128).all()


def test_brightness_table():
    img = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, -1)
    want = np.minimum(255, np.floor(np.arange(256, dtype=np.float32) * np.float32(rc.ENHANCE))).astype(np.uint8)
    assert np.array_equal(rc.brightness(img, rc.ENHANCE)[..., 0].reshape(-1), want)


def test_weight_table_and_levels():
    w = rc.weight_table()
    assert (w.sum((2, 3)) == 32768).all() and w.min() >= 0 and w.max() == 32767
    assert w[0, 0].tolist() == [[32767, 0], [0, 1]] and w[16, 16].tolist() == [[8192, 8192], [8192, 8192]]
    assert float(np.float32(rc.SHEAR)) == float(np.float32(0.21)) and rc.TRANSLATE == 7.0 and round(rc.ROTATE, 9) == 21.0
    assert abs(rc.ENHANCE - 1.36) < 1e-12


def _pil_affine(img, minv):
    """PIL's affine transform under the same source map: PIL samples at a (x + 0.5) + b (y + 0.5) + c - 0.5"""
    a, b, c, d, e, f = minv
    data = (a, b, c - 0.5 * a - 0.5 * b + 0.5, d, e, f - 0.5 * d - 0.5 * e + 0.5)
    H, W = img.shape[:2]
    return np.array(Image.fromarray(img).transform((W, H), Image.AFFINE, data, Image.BILINEAR, fillcolor=(rc.FILL,) * 3))


@pytest.mark.parametrize("op", ["TranslateX", "TranslateY"])
@pytest.mark.parametrize("sign", [1, -1])
def test_translate_equals_pil_exactly(op, sign):
    for kind in (0, 1, 2):
        img = rc.source(kind)
        minv = rc.invert(rc.forward_matrix(op, sign * rc.TRANSLATE, *img.shape[:2]))
        assert np.array_equal(rc.warp(img, minv), _pil_affine(img, minv)), (op, sign, kind)


@pytest.mark.parametrize("op,mag", [("ShearX", rc.SHEAR), ("ShearY", rc.SHEAR), ("Rotate", rc.ROTATE)])
@pytest.mark.parametrize("sign", [1, -1])
def test_shear_and_rotate_against_pil_on_a_ramp(op, mag, sign):
    """A ramp of slope <= 4 grey levels per pixel (|d/dx| + |d/dy| per channel).  The restatement rounds the source position to 1/32 pixel
    per axis, PIL interpolates in floating point at the unrounded position: the positions differ by at most 1/64 + 1/2048 per axis, bounded
    here by 2/32 in total, so the values by at most slope * 2 / 32, and each side then rounds to an integer: + 1.  The bound follows from the
    quantisation, it is not a measured number.  Pixels whose 2 x 2 footprint touches the border are excluded (PIL clamps there, cv2 blends
    with the fill)."""
    H, W = 48, 40
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([3 * xx + yy, 2 * xx + 2 * yy + 10, 250 - xx - 3 * yy], -1)
    assert img.min() >= 0 and img.max() <= 255
    img = img.astype(np.uint8)
    slope = 4
    minv = rc.invert(rc.forward_matrix(op, sign * mag, H, W))
    got, pil = rc.warp(img, minv).astype(np.int64), _pil_affine(img, minv).astype(np.int64)
    sx, sy, _, _ = rc.source_map(minv, H, W)
    inner = (sx >= 1) & (sx + 1 <= W - 2) & (sy >= 1) & (sy + 1 <= H - 2)
    assert inner.mean() > 0.4
    err = np.abs(got - pil)[inner].max()
    print(f"{op} {sign:+d}: max |restatement - PIL| on {int(inner.sum())} interior pixels = {err}")
    assert err <= slope * 2 / 32 + 1
    assert (got[(sx >= W) | (sx + 1 < 0) | (sy >= H) | (sy + 1 < 0)] == rc.FILL).all()


def test_rotation_corners_read_the_fill():
    img = rc.source(2)
    out = rc.apply_op(img, rc.code("Rotate"), rc.ROTATE)
    assert (out[0, 0] == rc.FILL).all() and (out[-1, -1] == rc.FILL).all() and not (out[10, 10] == rc.FILL).all()


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data():
    from fiber_amd import data
    return data


def test_plan_is_a_pure_function_of_shapes_and_seed(data):
    t = data.DeviceRandAugTransform(24)
    shapes = [(37, 53), (64, 48), (21, 21), (480, 640)] * 4
    a, b = t.plan(shapes, 1234), t.plan(shapes, 1234)
    assert a.dtype == t.plan_dtype and a.tobytes() == b.tobytes()
    assert a.tobytes() != t.plan(shapes, 1235).tobytes()
    assert t.plan(shapes[:5], 1234).tobytes() == a[:5].tobytes()           # sample i does not depend on the batch around it
    assert any(a[i].tobytes() != a[i + 4].tobytes() for i in range(4))      # ... but on its index
    assert set(a.dtype.names) == {"top", "left", "h", "w", "flip", "op", "arg"} and a["op"].shape == (16, 2)


def test_plan_arguments(data):
    t = data.DeviceRandAugTransform(24)
    p = t.plan([(40, 50)] * 4000, 99)
    for name in rc.OPS:
        sel = p["op"] == rc.code(name)
        args = np.unique(p["arg"][sel])
        if name in ("ShearX", "ShearY"):
            assert args.tolist() == [-rc.SHEAR, rc.SHEAR]
        elif name in ("TranslateX", "TranslateY"):
            assert args.tolist() == [-rc.TRANSLATE, rc.TRANSLATE]
        elif name == "Rotate":
            assert args.tolist() == [-rc.ROTATE, rc.ROTATE]
        elif name in ("Brightness", "Sharpness"):
            assert args.tolist() == [rc.ENHANCE]
        else:
            assert args.tolist() == [0.0]
    assert (p["arg"][p["op"] == rc.SKIP] == 0).all()
    for name in rc.GEOMETRIC:                                                # the matrices handed to the device are the restatement's
        for sign in (1, -1):
            arg = sign * {"S": rc.SHEAR, "T": rc.TRANSLATE, "R": rc.ROTATE}[name[0]]
            assert list(data.warp_affine_inverse(data.randaug_forward_matrix(name, arg, 30))) == rc.invert(rc.forward_matrix(name, arg, 30, 30))
    assert np.array_equal(data.bilinear_weight_table().astype(np.int64).reshape(32, 32, 2, 2), rc.weight_table())


def test_crop_boxes(data):
    t = data.DeviceRandAugTransform(24)
    shapes = [(37, 53), (64, 48), (21, 21), (480, 640), (333, 500), (3, 4)] * 200
    p = t.plan(shapes, 7)
    for (H, W), r in zip(shapes, p):
        top, left, h, w = int(r["top"]), int(r["left"]), int(r["h"]), int(r["w"])
        assert 0 <= top and 0 <= left and 0 < h and 0 < w and top + h <= H and left + w <= W
        # w = round(sqrt(area r)), h = round(sqrt(area / r)) with area / (H W) in [0.5, 1] and r in [3/4, 4/3]: each side is within half a
        # pixel of its unrounded value, which bounds the area and the aspect of every accepted box (the fallback is the whole image here)
        assert (w - 0.5) * (h - 0.5) <= H * W and (w + 0.5) * (h + 0.5) >= 0.5 * H * W
        assert (w - 0.5) / (h + 0.5) <= 4 / 3 and (w + 0.5) / (h - 0.5) >= 3 / 4
    assert len({(int(r["top"]), int(r["left"])) for r in p[3::6]}) > 150      # the position is drawn, not fixed
    # the fallback: no box of ratio in [3/4, 4/3] and area >= half fits a 10 x 100 strip -> torchvision's ratio-clamped centre crop
    q = t.plan([(10, 100), (100, 10)], 3)
    assert [tuple(int(q[0][k]) for k in ("top", "left", "h", "w"))] == [(0, 43, 10, 13)]
    assert [tuple(int(q[1][k]) for k in ("top", "left", "h", "w"))] == [(43, 0, 13, 10)]


def test_plan_frequencies(data):
    """20 000 planned samples: op and slot frequencies within 4 standard errors of the reference's distribution"""
    n = 20000
    t = data.DeviceRandAugTransform(24, flip_prob=0.3)
    p = t.plan([(30, 40)] * n, 2024)

    def within(count, total, prob):
        return abs(count / total - prob) <= 4 * math.sqrt(prob * (1 - prob) / total)

    assert within(int(p["flip"].sum()), n, 0.3)
    for s in range(2):
        assert within(int((p["op"][:, s] == rc.SKIP).sum()), n, 0.5)
        for name in rc.OPS:
            assert within(int((p["op"][:, s] == rc.code(name)).sum()), n, 0.5 / 10), (s, name)
        for name in rc.GEOMETRIC:
            sel = p["op"][:, s] == rc.code(name)
            assert within(int((p["arg"][sel, s] < 0).sum()), int(sel.sum()), 0.5), (s, name)
    both = (p["op"][:, 0] >= 0) & (p["op"][:, 1] >= 0)                     # the slots are independent
    assert within(int(both.sum()), n, 0.25)
    assert within(int((p["op"][both, 0] == p["op"][both, 1]).sum()), int(both.sum()), 0.1)


def test_a_subset_of_ops_and_unsupported_ones(data):
    t = data.DeviceRandAugTransform(24, augs=("Identity", "Rotate"), N=3)
    p = t.plan([(30, 40)] * 500, 5)
    assert p["op"].shape == (500, 3) and set(np.unique(p["op"]).tolist()) == {rc.SKIP, 0, rc.code("Rotate")}
    for name in ("Solarize", "Color", "Contrast", "Posterize"):
        with pytest.raises(NotImplementedError, match=name):
            data.DeviceRandAugTransform(24, augs=("Identity", name))
    with pytest.raises(ValueError):
        data.DeviceRandAugTransform(24, augs=("Cutout",))


def test_keys_to_transforms(data):
    from fiber_amd.config import named_config
    val, train = data.keys_to_transforms(["albef", "albef_randaug"], size=96)
    assert type(val) is data.DeviceImageTransform and type(train) is data.DeviceRandAugTransform
    assert val.size == 96 and train.size == 96 and train.N == 2 and train.M == 7 and train.augs == rc.OPS
    assert data.keys_to_transforms(["albef_randaug"])[0].size == 384
    with pytest.raises(KeyError):
        data.keys_to_transforms(["pixelbert"])
    cfg = named_config("task_finetune_irtr_itm_coco")
    train, val = (data.keys_to_transforms(cfg[k], cfg["image_size"])[0] for k in ("train_transform_keys", "val_transform_keys"))
    assert type(train) is data.DeviceRandAugTransform and type(val) is data.DeviceImageTransform and train.size == val.size == 384
