"""GPU tests of grounding training: each kernel of csrc/atss.hip alone through the C ABI against the fp64 restatement of tests/atss_cases.py
on NaN / -7-filled outputs with guard words, the zero-positive cases, bitwise repeatability, hipGraph capture (nothing synchronises), ABI
refusals, views through the ops wrappers, and VLDyHeadModule in training mode on the ground_small head weights.  Every test prints the
constant it needed (FIBER_ATSS_CALIBRATE=<file> collects them)."""
import ctypes
import json
import os

import pytest
import torch

import atss_cases as ac
import ground_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
G3 = (0.7, 0.3, 1.3)                                        # upstream gradients of the three sums
_CAL = os.environ.get("FIBER_ATSS_CALIBRATE")
_needed = {}


def _note(key, value):
    _needed[key] = max(_needed.get(key, 0.0), float(value))
    print(f"needs {key} {float(value):.3f}")
    if _CAL:
        with open(_CAL, "w") as f:
            json.dump(_needed, f, indent=1)


def _within(key, name, got, ref, mag):
    n = ac.need(got, ref, mag)
    _note(key, n)
    assert n <= ac.CONST[key], f"{name}: needs {key} {n:.2f} > {ac.CONST[key]}"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from fiber_amd import lib
    lib.load()
    return lib


_cache = {}


def _case(case):
    """device inputs, targets and the fp64 restatement (assignment, losses, gradients), once per case"""
    if case not in _cache:
        x = ac.inputs(case)
        t = ac.packed(case, x)
        anchors = ac.anchors()
        a = ac.assign_torch(anchors, t)
        x = ac.mark_edge(case, x, a["matched"])
        l = ac.losses_torch(x["bbox_reg"], x["centerness"], anchors, a["labels"], a["reg_targets"], grads=G3)
        dev = lambda v: v.to(DEV) if torch.is_tensor(v) else [u.to(DEV) for u in v] if isinstance(v, list) else v     # noqa: E731
        off = [0]
        for al in anchors:
            off.append(off[-1] + al.shape[0])
        _cache[case] = dict(x={k: dev(v) for k, v in x.items()}, t=t.to(DEV), anchors=[al.to(DEV) for al in anchors],
                            an=torch.cat(anchors).to(DEV), a={k: dev(v) for k, v in a.items()}, l={k: dev(v) for k, v in l.items()},
                            off=off, hoff=(ctypes.c_int * len(off))(*off))
    return _cache[case]


def _guarded(n, dtype, fill):
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[:n]


def _intact(buf, n, fill):
    tail = buf[n:]
    return bool(torch.isnan(tail).all()) if isinstance(fill, float) and fill != fill else bool((tail == fill).all())


NAN = float("nan")


@pytest.mark.parametrize("case", list(ac.CASES))
def test_candidates_kernel(lib, case):
    k = _case(case)
    t, a = k["t"], k["a"]
    B, G = t.labels.shape
    K = lib.plain("fiber_atss_num_candidates", k["hoff"], 5, ac.TOPK)
    assert K == ac.K_TOTAL == a["cand_idx"].shape[2]
    bi, idx = _guarded(B * G * K, torch.int32, -7)
    bf, iou = _guarded(B * G * K, torch.float32, NAN)
    lib.call("fiber_atss_candidates_f32", lib.ptr(k["an"]), k["hoff"], 5, lib.ptr(t.boxes), lib.ptr(t.num_gt), lib.ptr(idx), lib.ptr(iou),
             B, G, ac.A_TOTAL, ac.TOPK)
    idx, iou = idx.view(B, G, K), iou.view(B, G, K)
    live = torch.arange(G, device=DEV)[None, :] < t.num_gt[:, None]
    assert torch.equal(idx[live], a["cand_idx"][live]), f"{case}: candidates (order: ascending distance, then anchor index)"
    assert bool((idx[~live] == -7).all()) and bool(torch.isnan(iou[~live]).all()), "padding rows are not touched"
    # IoU <= 1 from six roundings of its operation order: 8 eps absolute
    assert float((iou[live].double() - a["cand_iou"][live]).abs().max()) <= 8 * ac.EPS if bool(live.any()) else True
    assert _intact(bi, B * G * K, -7) and _intact(bf, B * G * K, NAN)


def _ref_key(a, B, A):
    """the key the resolve kernel must produce from the restatement's candidates rounded to fp32"""
    m = a["matched"]
    G, K = a["cand_idx"].shape[1:]
    iou32 = a["cand_iou"].float()
    key = torch.zeros((B, A), dtype=torch.int64, device=DEV)
    for b, i in (m >= 0).nonzero().tolist():
        g = int(m[b, i])
        j = (a["cand_idx"][b, g] == i).nonzero().flatten()
        bits = int(iou32[b, g, j[0]].view(torch.int32))
        key[b, i] = (bits << 32) | (0xFFFFFFFF - g)
    return key


@pytest.mark.parametrize("case", list(ac.CASES))
def test_resolve_kernel(lib, case):
    k = _case(case)
    t, a = k["t"], k["a"]
    B, G = t.labels.shape
    A, K = ac.A_TOTAL, ac.K_TOTAL
    bk, key = _guarded(B * A, torch.int64, -7)
    lib.call("fiber_atss_resolve_f32", lib.ptr(k["an"]), lib.ptr(t.boxes), lib.ptr(t.num_gt), lib.ptr(a["cand_idx"].contiguous()),
             lib.ptr(a["cand_iou"].float().contiguous()), lib.ptr(key), B, G, A, K)
    assert torch.equal(key.view(B, A), _ref_key(a, B, A)), f"{case}: keys (iou bits << 32 | 0xFFFFFFFF - gt)"
    assert _intact(bk, B * A, -7)


@pytest.mark.parametrize("case", list(ac.CASES))
def test_finalize_kernel(lib, case):
    k = _case(case)
    t, a = k["t"], k["a"]
    B, G = t.labels.shape
    A = ac.A_TOTAL
    key = _ref_key(a, B, A)
    bufs = [_guarded(B * A, torch.int32, -7), _guarded(B * A, torch.int32, -7), _guarded(B * A * 4, torch.float32, NAN),
            _guarded(B * A * ac.T, torch.uint8, 7), _guarded(B, torch.int32, -7)]
    lib.call("fiber_atss_finalize_f32", lib.ptr(k["an"]), lib.ptr(t.boxes), lib.ptr(t.labels), lib.ptr(t.positive_map), lib.ptr(key),
             *[lib.ptr(v) for _, v in bufs], B, G, A, ac.T)
    matched, labels, reg, tok, npos = (v for _, v in bufs)
    assert torch.equal(matched.view(B, A), a["matched"]) and torch.equal(labels.view(B, A), a["labels"]), f"{case}: matched / labels"
    assert torch.equal(tok.view(B, A, ac.T), a["token_targets"]) and torch.equal(npos, a["num_pos"]), f"{case}: token targets / num_pos"
    reg = reg.view(B, A, 4)
    assert not bool(torch.isnan(reg).any()) and bool((reg[a["matched"] < 0] == 0).all())
    _within("K_REG", case, reg, a["reg_targets"], a["reg_mag"])
    for (buf, v), fill in zip(bufs, (-7, -7, NAN, 7, -7)):
        assert _intact(buf, v.numel(), fill), f"{case}: guard overwritten"


@pytest.mark.parametrize("case", list(ac.CASES))
def test_assign_wrapper_exact(lib, case):
    from fiber_amd import ops
    k = _case(case)
    a = k["a"]
    got = ops.atss_assign(k["anchors"], k["t"], ac.TOPK)
    for name in ("matched", "labels", "num_pos", "token_targets"):
        assert torch.equal(getattr(got, name), a[name]), f"{case}: {name}"
    _within("K_REG", case, got.reg_targets, a["reg_targets"], a["reg_mag"])
    if case == "atss_ties":
        assert not bool((got.matched == 2).any()) and bool((got.matched == 1).any())


def _loss_fwd(lib, k, labels, reg_targets):
    B, A = labels.shape
    rows = [lib.plain("fiber_atss_loss_rows", B, k["off"][l + 1] - k["off"][l]) for l in range(5)]
    bp, part = _guarded(sum(rows) * 3, torch.float32, NAN)
    bw, w = _guarded(B * A, torch.float32, NAN)
    row0 = 0
    for l in range(5):
        lib.call("fiber_atss_loss_fwd_f32", lib.ptr(k["x"]["bbox_reg"][l]), lib.ptr(k["x"]["centerness"][l]), lib.ptr(k["an"]), lib.ptr(labels),
                 lib.ptr(reg_targets), lib.ptr(part), lib.ptr(w), B, A, k["off"][l + 1] - k["off"][l], k["off"][l], row0)
        row0 += rows[l]
    assert _intact(bp, sum(rows) * 3, NAN) and _intact(bw, B * A, NAN)
    sums = torch.empty(3, device=DEV)
    lib.call("fiber_fold_rows_f32", lib.ptr(part), lib.ptr(sums), row0, 3)
    return sums, w.view(B, A)


@pytest.mark.parametrize("case", list(ac.CASES))
def test_loss_forward_kernel(lib, case):
    k = _case(case)
    a, l = k["a"], k["l"]
    sums, w = _loss_fwd(lib, k, a["labels"], a["reg_targets"].float().contiguous())
    assert not bool(torch.isnan(w).any()) and bool((w[a["labels"] <= 0] == 0).all())
    _within("K_CTR", case, w, l["w"], l["ctr_mag"])
    _within("K_SUM", case, sums, l["sums"], l["sums_abs"])


@pytest.mark.parametrize("case", list(ac.CASES))
def test_loss_backward_kernel(lib, case):
    k = _case(case)
    a, l = k["a"], k["l"]
    B, A = a["labels"].shape
    tg = a["reg_targets"].float().contiguous()
    g = torch.tensor(G3, device=DEV)
    lo = 0
    for lv in range(5):
        reg, ctr = k["x"]["bbox_reg"][lv], k["x"]["centerness"][lv]
        n = k["off"][lv + 1] - k["off"][lv]
        br, dreg = _guarded(reg.numel(), torch.float32, NAN)
        bc, dctr = _guarded(ctr.numel(), torch.float32, NAN)
        lib.call("fiber_atss_loss_bwd_f32", lib.ptr(reg), lib.ptr(ctr), lib.ptr(k["an"]), lib.ptr(a["labels"]), lib.ptr(tg), lib.ptr(g),
                 lib.ptr(dreg), lib.ptr(dctr), B, A, n, k["off"][lv])
        dreg, dctr = dreg.view(reg.shape), dctr.view(ctr.shape)
        assert _intact(br, reg.numel(), NAN) and _intact(bc, ctr.numel(), NAN) and not bool(torch.isnan(dreg).any() | torch.isnan(dctr).any())
        un = (a["labels"][:, lo:lo + n] <= 0).view(B, 1, *reg.shape[2:])
        assert bool((dreg[un.expand_as(dreg)] == 0).all()) and bool((dctr[un] == 0).all()), f"{case} level {lv}: unassigned anchors"
        mag = l["grad_mag"][:, lo:lo + n].permute(0, 2, 1).reshape(reg.shape)
        _within("K_GRAD", f"{case} level {lv} d bbox_reg", dreg, l["d_bbox_reg"][lv], mag)
        _within("K_GRAD", f"{case} level {lv} d centerness", dctr, l["d_centerness"][lv], l["ctr_grad_mag"][:, lo:lo + n].reshape(ctr.shape))
        if case == "atss_edge" and lv == 0:
            clamped = reg[:, 2] / 5.0 > ac.CLIP
            assert int((clamped & ~un[:, 0]).sum()) >= 1 and bool((dreg[:, 2][clamped] == 0).all()), "the clamped coordinate has no gradient"
        lo += n


def _full(k, targets, x=None):
    """assignment + losses forward + backward through the wrappers -> every output"""
    from fiber_amd import ops
    from fiber_amd.modules.grounding_train import ATSSLossComputation
    x = k["x"] if x is None else x
    regs = [t.clone().requires_grad_(True) for t in x["bbox_reg"]]
    ctrs = [t.clone().requires_grad_(True) for t in x["centerness"]]
    a = ops.atss_assign(k["anchors"], targets, ac.TOPK)
    lc = ATSSLossComputation.__new__(ATSSLossComputation)
    lc.reg_loss_weight = ac.REG_LOSS_WEIGHT
    loss_reg, loss_ctr, _ = lc.box_losses(regs, ctrs, k["anchors"], a)
    grads = torch.autograd.grad(loss_reg + loss_ctr, regs + ctrs)
    return [a.matched, a.labels, a.reg_targets, a.token_targets, a.num_pos, loss_reg.detach(), loss_ctr.detach(), *grads]


@pytest.mark.parametrize("image", [0, 1])
def test_zero_positive_cases(lib, image):
    """atss_edge's image without gts, and its image whose only gt no anchor centre is positive for, each alone"""
    from fiber_amd.modules.grounding_train import GroundingTargets
    k = _case("atss_edge")
    t = k["t"]
    sl = slice(image, image + 1)
    alone = GroundingTargets(t.boxes[sl].contiguous(), t.labels[sl].contiguous(), t.num_gt[sl].contiguous(), t.positive_map[sl].contiguous())
    assert int(alone.num_gt[0]) == image
    x = {key: [u[sl].contiguous() for u in v] for key, v in k["x"].items() if key in ("bbox_reg", "centerness")}
    out = _full(k, alone, x)
    assert bool((out[0] == -1).all()) and int(out[4][0]) == 0 and bool((out[3][..., -1] == 1).all()) and int(out[3].sum()) == ac.A_TOTAL
    assert float(out[5]) == 0.0 and float(out[6]) == 0.0
    for gr in out[7:]:
        assert bool((gr == 0).all()) and not bool(torch.isnan(gr).any())


def test_two_runs_agree_bitwise(lib):
    for case in ("atss_edge", "atss_many"):
        k = _case(case)
        one, two = _full(k, k["t"]), _full(k, k["t"])
        assert all(torch.equal(u, v) for u, v in zip(one, two)), f"{case}: two runs differ"


def test_captured_in_one_graph(lib):
    """Assignment + losses forward + backward on one stream in one graph: a capture that breaks means something synchronised."""
    k = _case("atss_edge")
    want = _full(k, k["t"])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _full(k, k["t"])                                     # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = _full(k, k["t"])
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(got, want)), "replay differs from eager"


def test_abi_refusals(lib):
    k = _case("atss_small")
    t, a = k["t"], k["a"]
    B, G = t.labels.shape
    A, K = ac.A_TOTAL, ac.K_TOTAL
    idx, iou = torch.empty((B, G, K), dtype=torch.int32, device=DEV), torch.empty((B, G, K), device=DEV)
    good = [lib.ptr(k["an"]), k["hoff"], 5, lib.ptr(t.boxes), lib.ptr(t.num_gt), lib.ptr(idx), lib.ptr(iou), B, G, A, ac.TOPK]
    lib.call("fiber_atss_candidates_f32", *good)
    one = (ctypes.c_int * 2)(0, 1)
    for pos, val in ((0, None), (3, None), (0, lib.ptr(k["an"]) + 4), (5, lib.ptr(idx) + 2), (1, None)):
        bad = list(good)
        bad[pos] = val
        with pytest.raises(lib.FiberHipError):
            lib.call("fiber_atss_candidates_f32", *bad)
    with pytest.raises(lib.FiberHipError):                   # sum k_l = 1 < 2: the reference's std is NaN
        lib.call("fiber_atss_candidates_f32", lib.ptr(k["an"]), one, 1, lib.ptr(t.boxes), lib.ptr(t.num_gt), lib.ptr(idx), lib.ptr(iou), B, G, 1, ac.TOPK)
    assert lib.plain("fiber_atss_num_candidates", one, 1, ac.TOPK) == -1
    with pytest.raises(lib.FiberHipError):                   # offsets that do not end at A
        lib.call("fiber_atss_candidates_f32", lib.ptr(k["an"]), k["hoff"], 5, lib.ptr(t.boxes), lib.ptr(t.num_gt), lib.ptr(idx), lib.ptr(iou), B, G, A + 1, ac.TOPK)
    key = torch.empty((B, A), dtype=torch.int64, device=DEV)
    with pytest.raises(lib.FiberHipError):
        lib.call("fiber_atss_resolve_f32", lib.ptr(k["an"]), lib.ptr(t.boxes), lib.ptr(t.num_gt), lib.ptr(idx), lib.ptr(iou), lib.ptr(key), B, G, A, 1)
    with pytest.raises(lib.FiberHipError):
        lib.call("fiber_atss_resolve_f32", lib.ptr(k["an"]), lib.ptr(t.boxes), lib.ptr(t.num_gt), lib.ptr(idx), lib.ptr(iou), lib.ptr(key) + 4, B, G, A, K)
    with pytest.raises(lib.FiberHipError):
        lib.call("fiber_atss_resolve_f32", lib.ptr(k["an"]), None, lib.ptr(t.num_gt), lib.ptr(idx), lib.ptr(iou), lib.ptr(key), B, G, A, K)
    z = torch.zeros(B * A * ac.T + 64, dtype=torch.uint8, device=DEV)
    zi = torch.zeros(B * A * 4 + 64, dtype=torch.int32, device=DEV)
    zf = torch.zeros(B * A * 4 + 64, device=DEV)
    fin = [lib.ptr(k["an"]), lib.ptr(t.boxes), lib.ptr(t.labels), lib.ptr(t.positive_map), lib.ptr(key), lib.ptr(zi), lib.ptr(zi), lib.ptr(zf),
           lib.ptr(z), lib.ptr(zi), B, G, A, ac.T]
    for pos, val in ((13, 128), (8, None), (8, lib.ptr(z) + 8), (7, lib.ptr(zf) + 4), (4, None)):
        bad = list(fin)
        bad[pos] = val
        with pytest.raises(lib.FiberHipError):
            lib.call("fiber_atss_finalize_f32", *bad)
    reg, ctr = k["x"]["bbox_reg"][0], k["x"]["centerness"][0]
    tg = a["reg_targets"].float().contiguous()
    fwd = [lib.ptr(reg), lib.ptr(ctr), lib.ptr(k["an"]), lib.ptr(a["labels"]), lib.ptr(tg), lib.ptr(zf), None, B, A, 560, 0, 0]
    for pos, val in ((0, None), (4, lib.ptr(tg) + 4), (9, 800), (5, lib.ptr(zf) + 2)):
        bad = list(fwd)
        bad[pos] = val
        with pytest.raises(lib.FiberHipError):
            lib.call("fiber_atss_loss_fwd_f32", *bad)
    bwd = [lib.ptr(reg), lib.ptr(ctr), lib.ptr(k["an"]), lib.ptr(a["labels"]), lib.ptr(tg), lib.ptr(zf), lib.ptr(zf), lib.ptr(zf), B, A, 560, 0]
    for pos, val in ((5, None), (6, None), (2, lib.ptr(k["an"]) + 8), (11, 200)):
        bad = list(bwd)
        bad[pos] = val
        with pytest.raises(lib.FiberHipError):
            lib.call("fiber_atss_loss_bwd_f32", *bad)
    lib.call("fiber_atss_candidates_f32", None, k["hoff"], 5, None, None, None, None, 0, G, A, ac.TOPK)     # B == 0: nothing to do
    torch.cuda.synchronize()


def test_ops_wrappers_take_views(lib):
    from fiber_amd import ops
    from fiber_amd.modules.grounding_train import GroundingTargets
    k = _case("atss_small")
    t = k["t"]
    want = ops.atss_assign(k["anchors"], t, ac.TOPK)
    B, G = t.labels.shape
    wide = torch.zeros((B, G, 5), device=DEV)
    wide[:, :, 1:] = t.boxes                                # views at odd offsets
    pm = torch.zeros((B, G, ac.T + 1), dtype=torch.uint8, device=DEV)
    pm[:, :, 1:] = t.positive_map
    an0 = torch.zeros((561, 4), device=DEV)
    an0[1:] = k["anchors"][0]
    got = ops.atss_assign([an0[1:]] + k["anchors"][1:], GroundingTargets(wide[:, :, 1:], t.labels.long(), t.num_gt.long(), pm[:, :, 1:]), ac.TOPK)
    for name in ("matched", "labels", "reg_targets", "token_targets", "num_pos"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    regs = [torch.zeros(r.shape[0], 5, *r.shape[2:], device=DEV) for r in k["x"]["bbox_reg"]]
    for w, r in zip(regs, k["x"]["bbox_reg"]):
        w[:, 1:] = r
    a = ops.atss_box_losses(k["x"]["bbox_reg"], k["x"]["centerness"], k["anchors"], want)
    b = ops.atss_box_losses([w[:, 1:] for w in regs], k["x"]["centerness"], k["anchors"], want)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    with pytest.raises(lib.FiberHipError):                   # one anchor in all: sum k_l < 2
        ops.atss_assign([k["anchors"][0][:1]], t, ac.TOPK)


def _module_cfg():
    cfg = gc.head_cfg(convs=gc.SMALL["convs"])
    import detect_cases as dc
    d = dc.cfg_for("detect_small")
    c = ac.cfg()
    for key, v in vars(c.MODEL.RPN).items():
        setattr(cfg.MODEL.RPN, key, v)
    cfg.MODEL.ATSS = d.MODEL.ATSS
    cfg.MODEL.ATSS.TOPK, cfg.MODEL.ATSS.REG_LOSS_WEIGHT, cfg.MODEL.RPN_ONLY = ac.TOPK, ac.REG_LOSS_WEIGHT, True
    cfg.MODEL.DYHEAD.SCORE_AGG, cfg.TEST = "MEAN", d.TEST
    cfg.MODEL.DYHEAD.FUSE_CONFIG.TOKEN_ALPHA, cfg.MODEL.DYHEAD.FUSE_CONFIG.TOKEN_GAMMA = 0.25, 2.0
    cfg.MODEL.DYHEAD.FUSE_CONFIG.DOT_PRODUCT_TOKEN_LOSS_WEIGHT = 1.0
    return cfg


def test_vldyhead_module_training(lib):
    """VLDyHeadModule in training mode on the ground_small head weights with atss_small targets on five levels.  The reference cannot
    run where the head's outputs exist (they come from the device's bf16 tower, and a second run may round differently), so the four
    losses are held against the fp64 restatements fed the VERY tensors the loss evaluator consumed (captured from the one run of the
    head): tests/ground_cases.py's bounds for the token loss, K_SUM for the other two."""
    from fiber_amd.modules import VLDyHeadModule
    m = VLDyHeadModule(_module_cfg())
    gc.set_head_weights(m.head)
    m = m.to(DEV).train()
    g = torch.Generator().manual_seed(0)
    xs = [torch.randn(2, gc.C, h, w, generator=g).to(torch.bfloat16).float().to(DEV) for h, w in ac.SIZES]
    emb = gc.small_inputs()[1].to(DEV)
    mask = gc.text_mask(2, gc.SMALL["lens"], "small").to(DEV)
    k = _case("atss_small")
    seen = []
    inner = m.head.training_outputs
    m.head.training_outputs = lambda *a, **kw: (seen.append(inner(*a, **kw)), seen[-1])[1]
    losses = m(None, xs, {"embedded": emb, "masks": mask}, targets=k["t"])
    assert set(losses) == {"loss_reg", "loss_centerness", "loss_cls", "loss_dot_product_token"} and len(seen) == 1
    sum(losses.values()).backward()
    logits, regs, ctrs, q, proj, tbias = seen[0]
    a = k["a"]
    l = ac.losses_torch(regs, ctrs, k["anchors"], a["labels"], a["reg_targets"])
    n = max(float(a["num_pos"].sum()), 1.0)
    s, sa = l["sums"], l["sums_abs"]
    ks = ac.CONST["K_SUM"] * ac.EPS
    want_reg = ac.REG_LOSS_WEIGHT * float(s[0] / s[1])
    need_reg = abs(float(losses["loss_reg"]) - want_reg) / (ac.EPS * ac.REG_LOSS_WEIGHT * float(sa[0] / s[1]) * 2)
    need_ctr = abs(float(losses["loss_centerness"]) - float(s[2]) / n) / (ac.EPS * float(sa[2]) / n)
    _note("K_SUM", max(need_reg, need_ctr))
    assert need_reg <= ac.CONST["K_SUM"] and need_ctr <= ac.CONST["K_SUM"], (need_reg, need_ctr, ks)
    assert float(losses["loss_cls"]) == 0.0
    r = gc.backward64(q.detach().to(torch.bfloat16), proj.detach().to(torch.bfloat16), tbias.detach(), m.head.log_scale.detach(),
                      a["token_targets"], mask, 0.25, 2.0)
    tok_need = abs(float(losses["loss_dot_product_token"]) * n - float(r["loss"])) / float(r["loss_el"].abs().sum())
    print(f"needs SUM(token) 2^{torch.log2(torch.tensor(max(tok_need, 1e-30))):.2f}")
    assert tok_need <= gc.CONST["SUM"] + 2.0 ** -23, tok_need
    for name, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        if name.startswith("head.cls_logits."):
            assert bool((p.grad == 0).all()), f"{name}: loss_cls carries no gradient"
        if name.startswith("head.bbox_pred.") or name.startswith("head.centerness."):
            assert bool((p.grad != 0).any()), f"{name}: no gradient"
