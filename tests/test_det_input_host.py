"""The grounding input pipeline on the host (no GPU): the numpy restatements of tests/det_input_cases.py against PIL itself, the PIL-produced
fixtures and the reference-run box fixture; fiber_amd.data.det_resize_size against a hand-worked table; the host half of
DeviceDetectionTransform / device_collate_grounding (configuration, the seeded choices, id padding and the mask)."""
import numpy as np
import pytest
import torch

import det_input_cases as dc
from fiber_amd import data


# ---------------------------------------------------------------------------------------------------- the bilinear restatement
@pytest.mark.parametrize("name", list(dc.RESIZE_CASES))
def test_bilinear_matches_pil_fixture(name, golden):
    gold = golden(name)
    H, W, oh, ow = dc.RESIZE_CASES[name]
    assert tuple(int(v) for v in gold["shape"]) == (H, W, oh, ow)
    assert np.array_equal(dc.resize_bilinear_u8(dc.case_image(name), oh, ow), gold["resized"])


def test_bilinear_matches_pil_live():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(11)
    for name, (H, W, oh, ow) in dc.RESIZE_CASES.items():
        for img in (dc.case_image(name), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)):
            ref = np.asarray(Image.fromarray(img, "RGB").resize((ow, oh), Image.BILINEAR))
            assert np.array_equal(dc.resize_bilinear_u8(img, oh, ow), ref), name
    for H, W, oh, ow in [(2, 200, 1, 100), (120, 160, 200, 266), (7, 1, 3, 5)]:       # a sliver, a camera-shaped upscale, one column
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(img, "RGB").resize((ow, oh), Image.BILINEAR))
        assert np.array_equal(dc.resize_bilinear_u8(img, oh, ow), ref), (H, W, oh, ow)


def test_to_tensor_times_255_is_the_identity_on_bytes():
    """fl(fl(v / 255) * 255) == v for every byte: "bgr255" feeds Normalize the integers themselves"""
    v = np.arange(256, dtype=np.float32)
    assert np.array_equal((v / np.float32(255.0)) * np.float32(255.0), v)


def test_normalize_ref_channel_order():
    """mean / std are indexed by the channel AFTER the swap: a constant image maps to ((value of source channel 2 - c) - mean[c]) / std[c]"""
    img = np.zeros((2, 3, 3), np.uint8)
    img[..., 0], img[..., 1], img[..., 2] = 10, 20, 30
    out = dc.normalize_ref(img, False, "bgr255", dc.BGR255_MEAN, dc.BGR255_STD)
    want = (np.asarray([30, 20, 10], np.float32) - np.asarray(dc.BGR255_MEAN, np.float32)) / np.asarray(dc.BGR255_STD, np.float32)
    assert np.array_equal(out[:, 0, 0], want)
    ramp = np.arange(2 * 5 * 3, dtype=np.uint8).reshape(2, 5, 3)
    assert np.array_equal(dc.normalize_ref(ramp, True, "rgb", dc.RGB_MEAN, dc.RGB_STD),
                          dc.normalize_ref(ramp, False, "rgb", dc.RGB_MEAN, dc.RGB_STD)[:, :, ::-1])


# ---------------------------------------------------------------------------------------------------- Resize.get_size
@pytest.mark.parametrize("args,want", dc.SIZE_TABLE)
def test_det_resize_size_table(args, want):
    assert data.det_resize_size(*args) == want
    assert dc.get_size_ref(*args) == want


def test_det_resize_size_agrees_with_restatement_on_a_sweep():
    for w in (1, 2, 33, 47, 64, 100, 131, 200):
        for h in (2, 20, 61, 64, 97, 150):
            for size in (1, 48, 64, 80):
                for mx in (None, 90, 133):
                    assert data.det_resize_size(w, h, size, mx) == dc.get_size_ref(w, h, size, mx), (w, h, size, mx)


# ---------------------------------------------------------------------------------------------------- boxes
@pytest.mark.parametrize("name", list(dc.BOX_CASES))
def test_boxes_ref_matches_reference_fixture(name, golden):
    orig, new, flip = dc.BOX_CASES[name]
    got = dc.boxes_ref(dc.case_boxes(name), orig, new, flip)
    assert np.array_equal(got, golden(dc.BOX_GOLDEN)[name])


def test_box_params_are_the_reference_ratios():
    il = data.DetImageList(None, [(64, 87), (80, 113)], [(97, 131, True), (33, 47, False)])
    rows = il.box_params([3, 0])
    assert rows == [(87.0 / 131.0, 64.0 / 97.0, 1, 87.0, 3), (113.0 / 47.0, 80.0 / 33.0, 0, 113.0, 0)]


# ---------------------------------------------------------------------------------------------------- the transform's host half
def test_transform_reads_the_nodes_build_transforms_reads():
    t = data.DeviceDetectionTransform(dc.input_cfg(), is_train=True)
    assert t.min_size == (48, 64, 80) and t.max_size == 133 and t.flip_threshold == 2 ** 31 and (t.bgr, t.times255) == (1, 1)
    assert t.size_divisible == 32 and list(t.mean) == [np.float32(v) for v in dc.BGR255_MEAN]
    t = data.DeviceDetectionTransform(dc.input_cfg(mult=(32, 40)), is_train=True)
    assert t.min_size == (32, 40)                                       # AUGMENT.MULT_MIN_SIZE_TRAIN wins when non-empty
    t = data.DeviceDetectionTransform(dc.input_cfg(mult=(32, 40), fmt="rgb", mean=dc.RGB_MEAN, std=dc.RGB_STD), is_train=False)
    assert t.min_size == (48,) and t.flip_threshold == 0 and (t.bgr, t.times255) == (0, 0)      # MIN_SIZE_TEST, never flips, FORMAT wins
    with pytest.raises(NotImplementedError, match="FIX_RES"):
        data.DeviceDetectionTransform(dc.input_cfg(fix_res=True))
    with pytest.raises(NotImplementedError, match="VERTICAL_FLIP_PROB_TRAIN"):
        data.DeviceDetectionTransform(dc.input_cfg(vflip=0.5))
    data.DeviceDetectionTransform(dc.input_cfg(vflip=0.5), is_train=False)      # build_transforms reads it for training only
    with pytest.raises(ValueError, match="FORMAT"):
        data.DeviceDetectionTransform(dc.input_cfg(to_bgr255=False))


def test_choices_are_a_pure_function_of_seed_and_index():
    t = data.DeviceDetectionTransform(dc.input_cfg(), is_train=True)
    shapes = [(97, 131), (20, 30), (150, 40), (64, 64), (61, 200), (33, 47), (2, 200), (100, 64)] * 4
    a, b, c = t.plan(shapes, 1234), t.plan(shapes, 1234), t.plan(shapes, 1235)
    assert a == b and (a[0], a[1]) != (c[0], c[1])
    ref = dc.choices_ref(1234, shapes, (48, 64, 80), 133, 0.5)
    assert a[0] == [r[0] for r in ref] and a[1] == [r[1] for r in ref]
    assert 4 < sum(a[1]) < len(shapes) - 4                              # both outcomes of the flip occur
    assert len({dc.hash_u32(1234, 2 * i) % 3 for i in range(len(shapes))}) == 3
    Hp, Wp = a[2]
    assert Hp % 32 == 0 and Wp % 32 == 0 and 0 <= Hp - max(s[0] for s in a[0]) < 32 and 0 <= Wp - max(s[1] for s in a[0]) < 32
    # the same sample at another position of the batch draws from another counter
    assert data.hash_u32(99, 7) == dc.hash_u32(99, 7)
    ev = data.DeviceDetectionTransform(dc.input_cfg(divisible=0), is_train=False)
    sizes, flips, pad = ev.plan(shapes[:3], 5)
    assert not any(flips) and sizes == [dc.get_size_ref(W, H, 48, 133) for H, W in shapes[:3]]
    assert pad == (max(s[0] for s in sizes), max(s[1] for s in sizes))


# ---------------------------------------------------------------------------------------------------- collate, host part
def test_pad_input_ids_and_mask():
    ids = [torch.tensor([0, 11, 12, 2]), torch.tensor([0, 21, 22, 23, 24, 25, 2]), torch.tensor([0, 2])]
    tok = data.pad_input_ids(ids, 12, True)
    assert tok["input_ids"].shape == (3, 12) and tok["input_ids"].dtype == torch.int64 and tok["attention_mask"].dtype == torch.int64
    assert tok["input_ids"][0].tolist() == [0, 11, 12, 2] + [1] * 8
    assert tok["attention_mask"].sum(1).tolist() == [4, 7, 2]
    assert torch.equal(tok["attention_mask"], (tok["input_ids"] != 1).long())
    tok = data.pad_input_ids(ids, 12, False)                           # PAD_MAX false: the longest
    assert tok["input_ids"].shape == (3, 7) and tok["input_ids"][2].tolist() == [0, 2, 1, 1, 1, 1, 1]
    tok = data.pad_input_ids(ids, 5, True)                             # truncation=True
    assert tok["input_ids"].shape == (3, 5) and tok["input_ids"][1].tolist() == [0, 21, 22, 23, 24]
