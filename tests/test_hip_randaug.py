"""GPU tests of the training image transform (csrc/input.hip randaug_* kernels through data.DeviceRandAugTransform): hand-written plans
against the numpy restatement of tests/randaug_cases.py, the uint8 image before ToTensor and the fp32 output over the WHOLE batch with
np.array_equal -- integer work, single correctly rounded fp32 / fp64 operations and table look-ups: there is no tolerance."""
import numpy as np
import pytest
import torch

import randaug_cases as rc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = (24, 30)                                                  # 30 is no multiple of 4: 2700 bytes per image, a 4-byte tail behind the
                                                                  # 16-byte histogram loads, images 12 bytes apart from their pitch


@pytest.fixture(scope="module")
def data():
    assert torch.cuda.is_available()
    from fiber_amd import data, lib
    lib.load()
    return data


def _plan(t, cases):
    p = np.zeros(len(cases), t.plan_dtype)
    for i, (_, (box, flip, slots)) in enumerate(cases):
        p[i]["top"], p[i]["left"], p[i]["h"], p[i]["w"] = box
        p[i]["flip"] = int(flip)
        for s, (code, arg) in enumerate(slots):
            p[i]["op"][s], p[i]["arg"][s] = code, arg
    return p


def _device(imgs):
    """device tensors; every fifth image is a row-strided view of a wider one"""
    out = []
    for i, im in enumerate(imgs):
        if i % 5 == 3:
            H, W = im.shape[:2]
            wide = torch.zeros((H, W + 9, 3), dtype=torch.uint8, device=DEV)
            wide[:, 4:4 + W] = torch.from_numpy(im).to(DEV)
            out.append(wide[:, 4:4 + W])
            assert out[-1].stride(0) == 3 * (W + 9)
        else:
            out.append(torch.from_numpy(im).to(DEV))
    return out


def _check(data, cases, S):
    t = data.DeviceRandAugTransform(S)
    imgs, ref_u8, ref = rc.batch_ref(cases, S)
    out, u8 = t.apply(_device(imgs), _plan(t, cases), return_u8=True)
    got_u8, got = u8.cpu().numpy(), out.cpu().numpy()
    assert got_u8.shape == ref_u8.shape and got_u8.dtype == np.uint8 and got.shape == ref.shape and got.dtype == np.float32
    bad = [(b, cases[b][1][2], int((got_u8[b] != ref_u8[b]).sum())) for b in range(len(cases)) if not np.array_equal(got_u8[b], ref_u8[b])]
    assert not bad, bad
    assert np.array_equal(got, ref), [b for b in range(len(cases)) if not np.array_equal(got[b], ref[b])]
    return t, imgs, out


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("position", [0, 1])
def test_every_op_alone_in_a_slot(data, position, S):
    cases = rc.single_slot_cases(position, S)
    assert 12 <= len(cases) <= 16 and {c[1][2][position][0] for c in cases} == set(range(10))
    assert {np.sign(c[1][2][position][1]) for c in cases if c[1][2][position][0] >= 5} == {1.0, -1.0}
    _check(data, cases, S)


@pytest.mark.parametrize("S", SIZES)
def test_slot_two_sees_slot_one(data, S):
    cases = rc.pair_cases(S)
    assert 12 <= len(cases) <= 16
    # the cases are what they claim to be: the rotation's fill reaches the statistics, the checkerboard wraps, the flat image is flat
    rot = rc.crop_resize_flip(rc.source(2), cases[2][1][0], S, False)
    assert cases[2][1][2][0][0] == rc.code("Rotate") and (rc.apply_op(rot, *cases[2][1][2][0])[0, 0] == rc.FILL).all()
    chk = rc.crop_resize_flip(rc.source("checker"), cases[12][1][0], S, False)
    raw = rc.sharpness_raw(chk, rc.ENHANCE)
    assert raw.min() <= -1 and raw.max() >= 256
    assert len(np.unique(rc.crop_resize_flip(rc.source("flat"), cases[10][1][0], S, False).reshape(-1, 3), axis=0)) == 1
    _check(data, cases, S)


@pytest.mark.parametrize("S", SIZES)
def test_all_slots_skipped_is_crop_resize_flip_normalize(data, S):
    cases = rc.skipped_cases(S)
    assert len(cases) == 14 and {c[1][1] for c in cases} == {False, True}
    _, imgs, out = _check(data, cases, S)
    for b, (im, (_, (box, flip, _))) in enumerate(zip(imgs, cases)):
        want = rc.to_tensor_normalize(rc.crop_resize_flip(im, box, S, flip))
        assert np.array_equal(out[b].cpu().numpy(), want), b


def test_identity_crop_equals_the_validation_transform(data):
    S = 30
    imgs = [rc.source(k) for k in (0, 1, 2, "checker", "narrow")]
    t = data.DeviceRandAugTransform(S)
    p = np.zeros(len(imgs), t.plan_dtype)
    p["op"] = rc.SKIP
    for i, im in enumerate(imgs):
        p[i]["h"], p[i]["w"] = im.shape[:2]
    dev = _device(imgs)
    assert torch.equal(t.apply(dev, p), data.DeviceImageTransform(S)(dev))


def test_call_is_apply_of_plan_and_collate_runs(data):
    S = 24
    t = data.DeviceRandAugTransform(S)
    imgs = [rc.source(i % 3) for i in range(12)]
    dev = _device(imgs)
    a = t(dev, seed=321)
    p = t.plan([im.shape[:2] for im in imgs], 321)
    assert (p["op"] >= 0).sum() >= 6
    assert torch.equal(a, t.apply(dev, p)) and torch.equal(a, t(dev, seed=321)) and not torch.equal(a, t(dev, seed=322))
    cases = [(i % 3, ((int(r["top"]), int(r["left"]), int(r["h"]), int(r["w"])), bool(r["flip"]), list(zip(r["op"].tolist(), r["arg"].tolist()))))
             for i, r in enumerate(p)]
    assert np.array_equal(a.cpu().numpy(), rc.batch_ref(cases, S)[2])
    samples = [{"image": d, "text_ids": torch.tensor([0, 100 + i, 101, 2], device=DEV)} for i, d in enumerate(dev)]
    batch = data.device_collate(samples, t, seed=5, max_text_len=8)
    img = batch["image"][0]
    assert tuple(img.shape) == (12, 3, S, S) and img.dtype == torch.float32 and bool(torch.isfinite(img).all())
    assert tuple(batch["text_ids"].shape) == (12, 8)
    with pytest.raises(ValueError):
        t.apply(dev, p[:5])
    bad = p.copy()
    bad[0]["top"] = 1000
    with pytest.raises(ValueError):
        t.apply(dev, bad)
    with pytest.raises(ValueError):
        t.apply([d.float() for d in dev], p)


def test_launch_count_does_not_depend_on_the_ops(data, monkeypatch):
    """3 ABI calls (3 + 2 + 2 kernels) for N = 2, whatever was drawn: all skipped, or Equalize after Rotate on every sample"""
    from fiber_amd import lib
    calls = []
    real = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    S = 24
    t = data.DeviceRandAugTransform(S)
    imgs = [rc.source(i % 3) for i in range(4)]
    dev = _device(imgs)
    counts = []
    for slots in ([rc.slot(None), rc.slot(None)], [rc.slot("Rotate"), rc.slot("Equalize")], [rc.slot("Sharpness"), rc.slot("ShearX", -1)]):
        del calls[:]
        cases = [(i % 3, ((0, 0) + im.shape[:2], False, slots)) for i, im in enumerate(imgs)]
        out = t.apply(dev, _plan(t, cases))
        counts.append(list(calls))
        assert np.array_equal(out.cpu().numpy(), rc.batch_ref(cases, S)[2])
    assert counts[0] == ["fiber_crop_resize_flip_u8", "fiber_randaug_slot_u8", "fiber_randaug_slot_u8"]
    assert counts[1] == counts[0] and counts[2] == counts[0]
    del calls[:]
    t(dev, seed=9)
    assert calls == counts[0]                                       # the default path draws on the host and adds no call
