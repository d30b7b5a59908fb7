"""GPU tests of the FPN neck: each kernel of csrc/fpn.hip alone through the C ABI against the fp64 restatement of tests/fpn_cases.py, every
output element within its bound on NaN-filled outputs with guard elements; the mask kernel exactly; ABI refusals; ops.fpn_merge's autograd;
modules/fpn.py against the reference-run fixture tests/golden/fpn_neck.npz (eval, train replaying the recorded draws, gradients; rel-L2
within twice the bf16-rounding restatement's own distance, fpn_cases.BF16_DISTANCE); and the end-to-end GeneralizedVLRCNN."""
import numpy as np
import pytest
import torch

import fpn_cases as fc
from hip_util import assert_close, assert_elementwise

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from fiber_amd import lib as L
    L.load()
    return L


def _dev_bf(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(BF).to(DEV).contiguous()


def _nan_out(n):
    return torch.full((n + fc.GUARD,), fc.NAN_BF16, dtype=torch.int16, device=DEV)


def _read(name, buf, shape):
    """the output as fp64 on the host; the guard elements behind it must still be NaN"""
    n = int(np.prod(shape))
    assert bool((buf[n:] == fc.NAN_BF16).all()), f"{name}: guard elements overwritten"
    return buf[:n].view(BF).view(shape).double().cpu()


def _check(name, buf, ref_bound):
    ref, bound = ref_bound
    worst = assert_elementwise(name, _read(name, buf, ref.shape), torch.from_numpy(ref), torch.from_numpy(bound))
    print(f"{name}: worst |err| / bound {worst:.3f}")


def _mask_dev(x):
    return (torch.from_numpy(x["keep"]).to(DEV).contiguous(), torch.tensor([x["kept"]], dtype=torch.int32, device=DEV)) if "keep" in x else (None, None)


@pytest.mark.parametrize("with_keep", [False, True])
@pytest.mark.parametrize("name", list(fc.MERGE_CASES))
def test_merge_forward(lib, name, with_keep):
    B, H, W, Hc, Wc, C = fc.MERGE_CASES[name]
    x = fc.merge_inputs(name, with_keep)
    lat, co = _dev_bf(x["lateral"]), _dev_bf(x["coarse"])
    keep, kept = _mask_dev(x)
    n = B * H * W * C
    inner, dropped = _nan_out(n), _nan_out(n) if with_keep else None
    lib.call("fiber_fpn_merge_fwd_bf16", lib.ptr(lat), lib.ptr(co), lib.ptr(keep), lib.ptr(kept), lib.ptr(inner), lib.ptr(dropped), B, H, W, C, Hc, Wc)
    ref = fc.merge_fwd_ref(x)
    _check(f"{name} inner", inner, ref["inner"])
    if with_keep:
        _check(f"{name} dropped", dropped, ref["dropped"])


@pytest.mark.parametrize("terms", ["inner", "dropped", "both"])
@pytest.mark.parametrize("name", list(fc.MERGE_CASES))
def test_merge_backward(lib, name, terms):
    """with d_inner or d_dropped NULL, and with both; `inner` runs without keep at all"""
    B, H, W, Hc, Wc, C = fc.MERGE_CASES[name]
    use_inner, use_dropped = terms != "dropped", terms != "inner"
    x = fc.merge_inputs(name, use_dropped)
    di = _dev_bf(x["d_inner"]) if use_inner else None
    dd = _dev_bf(x["d_dropped"]) if use_dropped else None
    keep, kept = _mask_dev(x)
    d_lat, d_co = _nan_out(B * H * W * C), _nan_out(B * Hc * Wc * C)
    lib.call("fiber_fpn_merge_bwd_bf16", lib.ptr(di), lib.ptr(dd), lib.ptr(keep), lib.ptr(kept), lib.ptr(d_lat), lib.ptr(d_co), B, H, W, C, Hc, Wc)
    ref = fc.merge_bwd_ref(x, use_inner, use_dropped)
    _check(f"{name} d_lateral", d_lat, ref["d_lateral"])
    _check(f"{name} d_coarse", d_co, ref["d_coarse"])


def test_merge_refusals(lib):
    t = torch.zeros(4096, dtype=BF, device=DEV)
    keep = torch.ones(64, dtype=torch.uint8, device=DEV)
    kept = torch.ones(1, dtype=torch.int32, device=DEV)
    p = lib.ptr
    for C in (4, 12, 7):                                     # a C that is no multiple of 8 -> 1
        with pytest.raises(lib.FiberHipError, match="code 1"):
            lib.call("fiber_fpn_merge_fwd_bf16", p(t), p(t), None, None, p(t), None, 1, 4, 4, C, 2, 2)
        with pytest.raises(lib.FiberHipError, match="code 1"):
            lib.call("fiber_fpn_merge_bwd_bf16", p(t), None, None, None, p(t), p(t), 1, 4, 4, C, 2, 2)
    with pytest.raises(lib.FiberHipError, match="code 1"):   # dropped_out without keep / kept
        lib.call("fiber_fpn_merge_fwd_bf16", p(t), p(t), None, None, p(t), p(t), 1, 4, 4, 8, 2, 2)
    with pytest.raises(lib.FiberHipError, match="code 1"):   # keep without kept
        lib.call("fiber_fpn_merge_fwd_bf16", p(t), p(t), p(keep), None, p(t), p(t), 1, 4, 4, 8, 2, 2)
    with pytest.raises(lib.FiberHipError, match="code 1"):   # d_dropped without keep
        lib.call("fiber_fpn_merge_bwd_bf16", None, p(t), None, None, p(t), p(t), 1, 4, 4, 8, 2, 2)
    with pytest.raises(lib.FiberHipError, match="code 1"):   # a base at an odd element offset
        lib.call("fiber_fpn_merge_fwd_bf16", p(t[1:]), p(t), None, None, p(t), None, 1, 4, 4, 8, 2, 2)
    for block in (2, 4, 0):                                  # even (or no) block -> 1
        with pytest.raises(lib.FiberHipError, match="code 1"):
            lib.call("fiber_dropblock_mask_u8", p(keep), 0, 0, None, 0.1, block, p(keep), p(kept), 1, 8, 8)
    lib.call("fiber_fpn_merge_fwd_bf16", p(t), p(t), p(keep), p(kept), p(t.clone()), p(t.clone()), 1, 4, 4, 8, 2, 2)      # the accepted form


def _run_mask(lib, seeds, draw, seed, gamma, block, shape, garbage):
    B, H, W = shape
    n = B * H * W
    keep = torch.full((n + fc.GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    kept = torch.full((2,), garbage, dtype=torch.int32, device=DEV)
    lib.call("fiber_dropblock_mask_u8", lib.ptr(seeds), draw, seed, None, gamma, block, lib.ptr(keep), lib.ptr(kept), B, H, W)
    assert bool((keep[n:] == 0xAB).all()) and int(kept[1]) == garbage
    return keep[:n].view(shape).cpu().numpy(), int(kept[0])


@pytest.mark.parametrize("block", fc.MASK_BLOCKS)
@pytest.mark.parametrize("shape", fc.MASK_SHAPES)
def test_mask_kernel(lib, shape, block):
    """draw = 0 replaying given seeds and draw = 1 against the Python hash: seeds, keep and kept are exact; kept prefilled with garbage
    comes out right; a second launch with the same key gives the same bits"""
    n = int(np.prod(shape))
    g = np.random.default_rng(n * 10 + block)
    given = (g.random(shape) < 0.12).astype(np.uint8)
    sd = torch.cat([torch.from_numpy(given).reshape(-1), torch.full((fc.GUARD,), 7, dtype=torch.uint8)]).to(DEV)
    keep, kept = _run_mask(lib, sd, 0, 0, 0.5, block, shape, -12345)
    rk, rn = fc.mask_ref(given, block)
    assert np.array_equal(keep, rk) and kept == rn
    assert np.array_equal(sd.cpu().numpy(), np.concatenate([given.reshape(-1), np.full(fc.GUARD, 7, np.uint8)]))      # read only
    gamma = 0.25 if n < 100 else fc.DROP_PROB / block ** 2
    want = fc.hash_seeds(fc.MASK_SEED, shape, gamma)
    runs = []
    for garbage in (987654321, -1):
        sd = torch.full((n + fc.GUARD,), 7, dtype=torch.uint8, device=DEV)
        keep, kept = _run_mask(lib, sd, 1, fc.MASK_SEED, gamma, block, shape, garbage)
        assert bool((sd[n:] == 7).all())
        assert np.array_equal(sd[:n].view(shape).cpu().numpy(), want)
        rk, rn = fc.mask_ref(want, block)
        assert np.array_equal(keep, rk) and kept == rn
        runs.append((keep, kept))
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]


def test_dropblock_mask_op_draws_from_the_key_stream(lib):
    from fiber_amd import ops
    saved = dict(ops._seed_state)
    try:
        ops.manual_seed(11)
        k1, n1 = ops.dropblock_mask(2, 25, 33, 0.3, 3, DEV)
        k2, n2 = ops.dropblock_mask(2, 25, 33, 0.3, 3, DEV)
        ops.manual_seed(11)
        k3, n3 = ops.dropblock_mask(2, 25, 33, 0.3, 3, DEV)
    finally:
        ops._seed_state.update(saved)                        # the key stream is process-wide: leave it as it was found
    assert torch.equal(k1, k3) and int(n1) == int(n3) == int(k1.sum()) and not torch.equal(k1, k2)
    assert 0.5 < int(n1) / k1.numel() < 0.9                   # 1 - (1 - 0.3 / 9)^9 ~ 0.26 of the pixels dropped


@pytest.mark.parametrize("use", ["inner", "dropped", "both"])
def test_fpn_merge_autograd(lib, use):
    """ops.fpn_merge's gradients against the restatement with either output unused; the inputs arrive as non-contiguous views"""
    from fiber_amd import ops
    name = "odd_1_2_4"
    x = fc.merge_inputs(name, True)
    lat = _dev_bf(x["lateral"]).permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1).requires_grad_(True)      # NCHW memory
    co = _dev_bf(x["coarse"]).permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1).requires_grad_(True)
    assert not lat.is_contiguous()
    keep, kept = _mask_dev(x)
    inner, dropped = ops.fpn_merge(lat, co, keep, kept)
    fwd = fc.merge_fwd_ref(x)
    assert_elementwise("inner", inner.double().cpu().contiguous(), torch.from_numpy(fwd["inner"][0]), torch.from_numpy(fwd["inner"][1]))
    assert_elementwise("dropped", dropped.double().cpu().contiguous(), torch.from_numpy(fwd["dropped"][0]), torch.from_numpy(fwd["dropped"][1]))
    loss = 0.0
    if use != "dropped":
        loss = loss + (inner.float() * _dev_bf(x["d_inner"]).float()).sum()
    if use != "inner":
        loss = loss + (dropped.float() * _dev_bf(x["d_dropped"]).float()).sum()
    loss.backward()
    ref = fc.merge_bwd_ref(x, use != "dropped", use != "inner")
    assert_elementwise("d_lateral", lat.grad.double().cpu().contiguous(), torch.from_numpy(ref["d_lateral"][0]), torch.from_numpy(ref["d_lateral"][1]))
    assert_elementwise("d_coarse", co.grad.double().cpu().contiguous(), torch.from_numpy(ref["d_coarse"][0]), torch.from_numpy(ref["d_coarse"][1]))
    i2, d2 = ops.fpn_merge(lat.detach(), co.detach())
    assert d2 is None and torch.equal(i2, inner)


# ---- the module against the reference-run fixture ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def neck(lib, golden):
    from fiber_amd.modules.fpn import build_swint_fpn
    gold = golden(fc.GOLDEN)
    m = build_swint_fpn(fc.neck_cfg())
    m.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in gold.items() if k.startswith("w.")})
    return m.to(DEV), gold


def test_fpn_module_eval_vs_reference(neck):
    m, gold = neck
    maps, _ = fc.neck_inputs()
    m.eval()
    with torch.no_grad():
        out = m([t.to(DEV) for t in maps])
    assert isinstance(out, tuple) and len(out) == 5
    for n, o in zip(fc.OUT_NAMES, out):
        assert o.dtype == torch.float32 and tuple(o.shape) == gold["eval." + n].shape
        e = assert_close("eval." + n, o, torch.from_numpy(gold["eval." + n]), fc.gpu_tolerance("eval." + n))
        print(f"eval.{n}: rel-L2 {e:.3e} (allowed {fc.gpu_tolerance('eval.' + n):.3e})")
    res, text, c4 = m(([t.to(DEV) for t in maps], "text"))   # the VL backbones' tuple form
    assert text == "text" and c4 is None and all(torch.equal(a, b) for a, b in zip(res, out))


def test_fpn_module_train_and_gradients_vs_reference(neck):
    m, gold = neck
    maps, proj = fc.neck_inputs()
    m.train()
    m.zero_grad(set_to_none=True)
    xs = [t.to(DEV).requires_grad_(True) for t in maps]
    seeds = [torch.from_numpy(gold["draw.s16"]).to(DEV), torch.from_numpy(gold["draw.s8"]).to(DEV)]
    out = m(xs, seeds=seeds)
    sum((o * p.to(DEV)).sum() for o, p in zip(out, proj)).backward()
    for n, o in zip(fc.OUT_NAMES, out):
        e = assert_close("train." + n, o, torch.from_numpy(gold["train." + n]), fc.gpu_tolerance("train." + n))
        print(f"train.{n}: rel-L2 {e:.3e} (allowed {fc.gpu_tolerance('train.' + n):.3e})")
    assert xs[0].grad is None                                # the stride-4 map is never read
    for i, x in enumerate(xs[1:]):
        k = f"grad.x{i + 3}"
        e = assert_close(k, x.grad, torch.from_numpy(gold[k]), fc.gpu_tolerance(k))
        print(f"{k}: rel-L2 {e:.3e} (allowed {fc.gpu_tolerance(k):.3e})")
    floors = {"fpn_layer2.bias": fc.sum_floor(proj[0]), "fpn_layer3.bias": fc.sum_floor(proj[1]), "top_blocks.p7.bias": fc.sum_floor(proj[4])}
    for name, p in m.named_parameters():
        k = "grad." + name
        tol = fc.gpu_tolerance(k, floors.get(name, 0.0))
        assert p.grad is not None and p.grad.shape == p.shape, name
        e = assert_close(k, p.grad, torch.from_numpy(gold[k]), tol)
        print(f"{k}: rel-L2 {e:.3e} (allowed {tol:.3e})")
    m.eval()


def test_dropblock2d_module(lib):
    from fiber_amd.modules.fpn import DropBlock2D
    d = DropBlock2D(0.3, 3).to(DEV)
    g = np.random.default_rng(3)
    x = torch.from_numpy(g.standard_normal((2, 16, 13, 17)).astype(np.float32)).to(BF).float().to(DEV)
    seeds = torch.from_numpy((g.random((2, 13, 17)) < 0.05).astype(np.uint8))
    assert d.eval()(x) is x
    y = d.train()(x, seeds=seeds.to(DEV))
    keep, kept = fc.mask_ref(seeds.numpy(), 3)
    ref = x.double().cpu() * torch.from_numpy(keep).double()[:, None] * (keep.size / kept)
    bound = torch.from_numpy(fc.bf16_store(ref.numpy())) + fc.const(3) * fc.F32 * ref.abs()
    assert_elementwise("dropblock", y.double().cpu().contiguous(), ref.contiguous(), bound)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detector(lib):
    from fiber_amd.modules import GeneralizedVLRCNN
    from fiber_amd.modules.grounding_train import pack_targets
    torch.manual_seed(0)
    model = GeneralizedVLRCNN(fc.model_cfg()).to(DEV)
    g = np.random.default_rng(0)
    B, T = 2, 256
    images = torch.from_numpy(g.standard_normal((B, 3, 64, 96)).astype(np.float32)).to(DEV)
    ids = torch.from_numpy(g.integers(3, 50000, size=(B, T))).to(DEV)
    am = torch.zeros((B, T), dtype=torch.int64)
    am[0, :9], am[1, :14] = 1, 1
    ids[am.to(DEV) == 0] = 1
    pm = torch.zeros((3, T), dtype=torch.uint8)
    pm[0, 1:3], pm[1, 4], pm[2, 2:5] = 1, 1, 1
    targets = pack_targets([torch.tensor([[8.0, 6.0, 60.0, 50.0], [40.0, 20.0, 90.0, 60.0]]), torch.tensor([[10.0, 10.0, 80.0, 55.0]])],
                           [torch.tensor([1, 2]), torch.tensor([1])], pm, device=DEV)
    return model, images, {"input_ids": ids, "attention_mask": am.to(DEV)}, targets


def test_detector_train_step(detector):
    model, images, tok, targets = detector
    model.train()
    model.zero_grad(set_to_none=True)
    losses = model(images, targets=targets, tokenizer_input=tok)
    assert set(losses) == {"loss_reg", "loss_centerness", "loss_cls", "loss_dot_product_token"}
    assert all(bool(torch.isfinite(v)) for v in losses.values()), losses
    sum(losses.values()).backward()
    missing = [n for n, p in model.named_parameters() if p.requires_grad and p.grad is None]
    # Swin depths (2, 2, 2, 2): the stage-3 blocks 14.. that pair with text layers 6 - 9 do not exist, so those layers never run
    assert all(any(f".encoder.layer.{i}." in n for i in (6, 7, 8, 9)) for n in missing), missing[:8]
    for n, p in model.fusion_backbone.backbone.fpn.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0, n
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)
    assert all(p.grad is None for p in model.rpn.head.cls_logits.parameters())           # frozen under the dot-product token loss


def test_detector_eval_and_channels_last_handover(detector):
    from fiber_amd.modules import Detections
    model, images, tok, _ = detector
    model.eval()
    with torch.no_grad():
        det = model((images, [(64, 96), (60, 90)]), positive_map={1: [1, 2], 2: [4], 3: 7}, tokenizer_input=tok)
        assert isinstance(det, Detections)
        B, D = 2, model.cfg.MODEL.ATSS.DETECTIONS_PER_IMG
        assert det.boxes.shape == (B, D, 4) and det.scores.shape == (B, D) and det.labels.shape == (B, D) and det.count.shape == (B,)
        assert det.boxes.dtype == torch.float32 and det.labels.dtype == torch.int32 and len(det.to_list()) == B
        fb = model.fusion_backbone
        vis, lang, _ = fb(tok, images)
        assert [tuple(v.shape) for v in vis] == [(2, 256, 8, 12), (2, 256, 4, 6), (2, 256, 2, 3), (2, 256, 1, 2), (2, 256, 1, 1)]
        neck = fb.backbone.fpn
        fb.backbone.fpn = None
        try:
            stages, lang2, _ = fb(tok, images)               # the fpn=None return value: NCHW stage maps
        finally:
            fb.backbone.fpn = neck
        assert [tuple(s.shape) for s in stages] == [(2, 128, 16, 24), (2, 256, 8, 12), (2, 512, 4, 6), (2, 1024, 2, 3)]
        by_hand = neck(stages)
        for a, b in zip(vis, by_hand):
            assert a.dtype == b.dtype and torch.equal(a, b)   # bitwise: the channels-last hand-over changes no value
        assert torch.equal(lang["embedded"], lang2["embedded"])
