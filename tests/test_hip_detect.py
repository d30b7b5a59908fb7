"""GPU tests of grounding inference: each kernel of csrc/detect.hip alone against the fp64 restatement of tests/detect_cases.py on NaN-filled
outputs with guard words, the whole ATSSPostProcessor against the reference-run fixtures tests/golden/detect_*.npz (exact order of source
indices, labels and count; floats within the bound), bitwise repeatability, ABI refusals, views through the ops wrappers, VLDyHeadModule on
the ground_small head weights, and hipGraph capture.  Every test prints the constant it needed (FIBER_DETECT_CALIBRATE=<file> collects them)."""
import json
import os

import numpy as np
import pytest
import torch

import detect_cases as dc
import ground_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
_CAL = os.environ.get("FIBER_DETECT_CALIBRATE")
_needed = {}


def _note(key, value):
    _needed[key] = max(_needed.get(key, 0.0), float(value))
    print(f"needs {key} {float(value):.3f}")
    if _CAL:
        with open(_CAL, "w") as f:
            json.dump(_needed, f, indent=1)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from fiber_amd import lib
    lib.load()
    return lib


_cache = {}


def _case(case):
    """device inputs + the fp64 and fp32 restatements evaluated on the device, once per case"""
    if case not in _cache:
        c = dc.CASES[case]
        x = {k: [t.to(DEV) for t in v] for k, v in dc.inputs(case).items()}
        anchors = [a.to(DEV) for a in dc.anchors_for(case)]
        sizes = torch.tensor(c["image_sizes"], dtype=torch.float32, device=DEV)
        args = (x["logits"], x["bbox_reg"], x["centerness"], anchors, sizes, c["positive_map"], c["C"], c["agg"], c["thresh"], c["top_n"], c["nms"], c["D"])
        _cache[case] = dict(c=c, x=x, anchors=anchors, sizes=sizes, r64=dc.postprocess_torch(*args, dtype=torch.float64),
                            r32=dc.postprocess_torch(*args, dtype=torch.float32))
    return _cache[case]


def _guarded(n, dtype, fill):
    """a flat buffer of n + GUARD elements filled with `fill` -> (buffer, view of the first n)"""
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[:n]


def _guard_intact(buf, n, fill):
    tail = buf[n:]
    return bool(torch.isnan(tail).all()) if isinstance(fill, float) and fill != fill else bool((tail == fill).all())


def _check_scores(name, got, ref):
    live = ref >= 0
    assert torch.equal(got >= 0, live) and bool((got[~live] == -1).all()), f"{name}: the -1 pattern differs"
    err = (got.double() - ref).abs()[live]
    need = float((err / (dc.EPS * ref[live].abs().clamp_min(2.0 ** -20))).max()) if bool(live.any()) else 0.0
    _note("K_SCORE", need)
    assert need <= dc.CONST["K_SCORE"], f"{name}: scores need K_SCORE {need:.2f} > {dc.CONST['K_SCORE']}"


def _check_boxes(name, got, ref, mag):
    need = float(((got.double() - ref).abs() / (dc.EPS * torch.cat([mag, mag], -1)).clamp_min(1e-300)).max())
    _note("K_BOX", need)
    assert need <= dc.CONST["K_BOX"], f"{name}: boxes need K_BOX {need:.2f} > {dc.CONST['K_BOX']}"


@pytest.mark.parametrize("case", list(dc.CASES))
def test_scores_kernel_against_fp64(lib, case):
    k = _case(case)
    c = k["c"]
    ptr, idx = (t.to(DEV) for t in dc.csr(c["positive_map"], c["C"], c["v2"]))
    for l, (lg, ctr) in enumerate(zip(k["x"]["logits"], k["x"]["centerness"])):
        B, A, _ = lg.shape
        n = B * A * c["C"]
        buf, out = _guarded(n, torch.float32, float("nan"))
        lib.call("fiber_det_scores_f32", lib.ptr(lg), lib.ptr(ctr), lib.ptr(ptr), lib.ptr(idx), lib.ptr(out), B, A, dc.T, c["C"], c["thresh"],
                 int(c["agg"] == "MAX"))
        assert not bool(torch.isnan(out).any()) and _guard_intact(buf, n, float("nan")), f"{case} level {l}: unwritten output or guard overwritten"
        _check_scores(f"{case} level {l}", out.view(B, A, c["C"]), k["r64"]["dense"][l])


@pytest.mark.parametrize("case", list(dc.CASES))
def test_decode_kernel_against_fp64(lib, case):
    k = _case(case)
    c, B = k["c"], k["c"]["B"]
    ks = [dc.level_k(c["top_n"], a.shape[0], c["C"]) for a in k["anchors"]]
    N = sum(ks) + 7                                       # a slice past the last level stays untouched
    bufs = [_guarded(B * N * 4, torch.float32, float("nan")), _guarded(B * N, torch.float32, float("nan")),
            _guarded(B * N, torch.int32, -77), _guarded(B * N, torch.int32, -77)]
    boxes, scores, labels, source = bufs[0][1].view(B, N, 4), bufs[1][1].view(B, N), bufs[2][1].view(B, N), bufs[3][1].view(B, N)
    off = 0
    for l, kk in enumerate(ks):
        dense = k["r64"]["dense"][l].reshape(B, -1)
        val, flat = torch.topk(dense, kk, dim=1)
        val32 = val.float().contiguous()
        lib.call("fiber_det_decode_f32", lib.ptr(val32), lib.ptr(flat), lib.ptr(k["x"]["bbox_reg"][l]), lib.ptr(k["anchors"][l]), lib.ptr(k["sizes"]),
                 lib.ptr(boxes), lib.ptr(scores), lib.ptr(labels), lib.ptr(source), B, kk, k["anchors"][l].shape[0], c["C"], N, off, l, 0.0)
        rb, rs, rl, rsrc, mag = dc.decode(val32.double(), flat, k["x"]["bbox_reg"][l], k["anchors"][l], k["sizes"], c["C"], l)
        sl = slice(off, off + kk)
        assert torch.equal(labels[:, sl], rl) and torch.equal(source[:, sl], rsrc), f"{case} level {l}: labels / source"
        _check_scores(f"{case} level {l} sqrt", scores[:, sl], rs)
        live = rs >= 0
        _check_boxes(f"{case} level {l}", boxes[:, sl][live], rb[live], mag[live])
        assert bool((boxes[:, sl][~live] == 0).all())
        off += kk
    assert bool(torch.isnan(scores[:, off:]).all()) and bool((labels[:, off:] == -77).all()) and bool(torch.isnan(boxes[:, off:]).all())
    for (buf, v), fill in zip(bufs, (float("nan"), float("nan"), -77, -77)):
        assert _guard_intact(buf, v.numel(), fill), f"{case}: guard overwritten"


def _sorted_candidates(k):
    r = k["r32"]
    return r["cand_boxes"].contiguous(), r["cand_scores"].contiguous(), r["cand_labels"].contiguous(), r["cand_source"].contiguous()


@pytest.mark.parametrize("case", list(dc.CASES))
def test_mask_kernel_bit_for_bit(lib, case):
    k = _case(case)
    boxes, scores, labels, _ = _sorted_candidates(k)
    B, N = scores.shape
    NB = (N + 63) // 64
    sup = dc.suppression(boxes.double(), scores.double(), labels, k["c"]["nms"])
    iou = dc.iou_matrix(boxes.double())
    pair = (labels[:, :, None] == labels[:, None, :]) & (scores >= 0)[:, :, None] & (scores >= 0)[:, None, :]
    margin = float((iou[pair] - k["c"]["nms"]).abs().min())
    assert margin >= 1e-5, f"{case}: an IoU within {margin:.1e} of the threshold: the inputs are not decisive"
    want = dc.mask_words(sup)
    SENT = 0x5A5A5A5A5A5A5A5A
    buf, mask = _guarded(B * N * NB, torch.int64, SENT)
    lib.call("fiber_det_nms_mask", lib.ptr(boxes), lib.ptr(scores), lib.ptr(labels), lib.ptr(mask), B, N, k["c"]["nms"])
    mask = mask.view(B, N, NB)
    upper = (torch.arange(NB, device=DEV)[None, :] >= (torch.arange(N, device=DEV) // 64)[:, None])[None].expand(B, -1, -1)
    assert torch.equal(mask[upper], want[upper]), f"{case}: mask words differ"
    assert bool((mask[~upper] == SENT).all()), f"{case}: a block below the diagonal was written"
    assert _guard_intact(buf, B * N * NB, SENT)
    assert int((want != 0).sum()) > 0 or case == "detect_edge"


@pytest.mark.parametrize("case", list(dc.CASES))
@pytest.mark.parametrize("D", [100, 7])
def test_select_kernel_exact(lib, case, D):
    k = _case(case)
    boxes, scores, labels, source = _sorted_candidates(k)
    B, N = scores.shape
    sup = dc.suppression(boxes.double(), scores.double(), labels, k["c"]["nms"])
    mask = dc.mask_words(sup).contiguous()
    want = dc.select(boxes, scores, labels, source, dc.greedy_keep(sup, scores, D), D)
    bufs = [_guarded(B * D * 4, torch.float32, float("nan")), _guarded(B * D, torch.float32, float("nan")), _guarded(B * D, torch.int32, -77),
            _guarded(B * D, torch.int32, -77), _guarded(B, torch.int32, -77)]
    lib.call("fiber_det_nms_select", lib.ptr(boxes), lib.ptr(scores), lib.ptr(labels), lib.ptr(source), lib.ptr(mask),
             *[lib.ptr(v) for _, v in bufs], B, N, D)
    shapes = [(B, D, 4), (B, D), (B, D), (B, D), (B,)]
    for name, (buf, v), w, shp, fill in zip(("boxes", "scores", "labels", "source", "count"), bufs, want, shapes, (float("nan"),) * 2 + (-77,) * 3):
        assert torch.equal(v.view(shp), w), f"{case} D={D}: {name} differ"
        assert _guard_intact(buf, v.numel(), fill), f"{case}: guard of {name} overwritten"



# ---- the NMS kernels alone past the select kernel's first bitmap slot -----------------------------------------------------------------
_big = {}


def _big_case():
    """dc.big_candidates on the device with its fp64 suppression matrix, mask words and full greedy walk, computed once"""
    if not _big:
        boxes, scores, labels, source = dc.big_candidates(DEV)
        sup = dc.suppression(boxes.double(), scores.double(), labels, dc.BIG["nms"])
        _big.update(boxes=boxes, scores=scores, labels=labels, source=source, sup=sup, words=dc.mask_words(sup).contiguous())
    return _big


def test_mask_kernel_large_n(lib):
    k = _big_case()
    B, N = k["scores"].shape
    NB = (N + 63) // 64
    assert N % 64 and NB > 128, "the case reaches the third bitmap slot and ends inside a block"
    SENT = 0x5A5A5A5A5A5A5A5A
    buf, mask = _guarded(B * N * NB, torch.int64, SENT)
    lib.call("fiber_det_nms_mask", lib.ptr(k["boxes"]), lib.ptr(k["scores"]), lib.ptr(k["labels"]), lib.ptr(mask), B, N, dc.BIG["nms"])
    mask = mask.view(B, N, NB)
    upper = (torch.arange(NB, device=DEV)[None, :] >= (torch.arange(N, device=DEV) // 64)[:, None])[None].expand(B, -1, -1)
    assert torch.equal(mask[upper], k["words"][upper]), "mask words differ"
    assert bool((mask[~upper] == SENT).all()) and _guard_intact(buf, B * N * NB, SENT)
    iou = dc.iou_matrix(k["boxes"][:1].double())[0]
    ties = (iou == 0.5) & (k["labels"][0][:, None] == k["labels"][0][None, :])
    assert bool(ties.any()) and not bool((k["sup"][0] & ties).any()), "exact ties at the threshold exist and are not suppressed"


@pytest.mark.parametrize("D", [8300, 5000])
def test_select_kernel_large_n(lib, D):
    k = _big_case()
    B, N = k["scores"].shape
    keep = dc.greedy_keep(k["sup"], k["scores"], D)
    for b in range(B):                                       # what the case must reach: decisions and suppression across the slot boundaries
        kept = keep[b].nonzero().flatten()
        s = k["sup"][b]
        assert int(kept.max()) >= 4096 + 64 and bool(s[kept[kept < 4096]][:, 4096:].any()), "slot 0 -> 1"
        if D == N:
            assert int(kept.max()) >= 8192 and bool(s[kept[(kept >= 4096) & (kept < 8192)]][:, 8192:].any()) and \
                bool(s[kept[kept < 4096]][:, 8192:].any()), "slots 0, 1 -> 2"
            assert int(keep[b].sum()) < D
        else:
            assert int(keep[b].sum()) == D, "the walk stops at D inside slot 1"
    want = dc.select(k["boxes"], k["scores"], k["labels"], k["source"], keep, D)
    bufs = [_guarded(B * D * 4, torch.float32, float("nan")), _guarded(B * D, torch.float32, float("nan")), _guarded(B * D, torch.int32, -77),
            _guarded(B * D, torch.int32, -77), _guarded(B, torch.int32, -77)]
    lib.call("fiber_det_nms_select", lib.ptr(k["boxes"]), lib.ptr(k["scores"]), lib.ptr(k["labels"]), lib.ptr(k["source"]), lib.ptr(k["words"]),
             *[lib.ptr(v) for _, v in bufs], B, N, D)
    for name, (buf, v), w, shp, fill in zip(("boxes", "scores", "labels", "source", "count"), bufs, want,
                                            [(B, D, 4), (B, D), (B, D), (B, D), (B,)], (float("nan"),) * 2 + (-77,) * 3):
        assert torch.equal(v.view(shp), w), f"D={D}: {name} differ"
        assert _guard_intact(buf, v.numel(), fill), f"guard of {name} overwritten"
    from fiber_amd import ops                                # and both kernels together through the wrapper
    got = ops.nms_ml(k["boxes"], k["scores"], k["labels"], k["source"], dc.BIG["nms"], D)
    assert all(torch.equal(u, v) for u, v in zip(got, want))


def test_strict_greater_on_an_exact_tie(lib):
    """The hand-made candidates of the host test: IoU(0, 1) = 50 / 100, exactly 0.5 in fp32.  Strict > keeps box 1; >= would drop it.
    At NMS 0.4 (not a tie) boxes 1 and 3 go: 0.5 and 60 / 140 with the +1 convention, which 45 / 117 without it would not reach."""
    from fiber_amd import ops
    boxes = torch.tensor([[[0, 0, 9, 9], [0, 0, 9, 4], [20, 20, 29, 29], [24, 20, 33, 29]]], dtype=torch.float32, device=DEV)
    scores = torch.tensor([[0.9, 0.8, 0.7, 0.6]], device=DEV)
    labels = torch.ones((1, 4), dtype=torch.int32, device=DEV)
    source = torch.arange(4, dtype=torch.int32, device=DEV)[None]
    mask = torch.full((1, 4, 1), -1, dtype=torch.int64, device=DEV)
    lib.call("fiber_det_nms_mask", lib.ptr(boxes), lib.ptr(scores), lib.ptr(labels), lib.ptr(mask), 1, 4, 0.5)
    assert mask.flatten().tolist() == [0, 0, 0, 0]
    out = ops.nms_ml(boxes, scores, labels, source, 0.5, 10)
    assert int(out[4]) == 4 and out[3][0, :4].tolist() == [0, 1, 2, 3]
    out = ops.nms_ml(boxes, scores, labels, source, 0.4, 10)
    assert int(out[4]) == 2 and out[3][0, :2].tolist() == [0, 2]
    labels[0, 1] = 2                                         # label-aware: another label is never suppressed
    assert ops.nms_ml(boxes, scores, labels, source, 0.4, 10)[3][0, :3].tolist() == [0, 1, 2]


def _post(case):
    from fiber_amd.modules.grounding_inference import BoxCoder, make_atss_postprocessor
    return make_atss_postprocessor(dc.cfg_for(case), BoxCoder())


def _forward(post, k):
    return post(k["x"]["bbox_reg"], k["x"]["centerness"], k["sizes"], k["anchors"], k["x"]["logits"], k["c"]["positive_map"])


@pytest.mark.parametrize("case", list(dc.CASES))
def test_pipeline_against_reference_fixture(lib, golden, case):
    gold, k = golden(case), _case(case)
    det = _forward(_post(case), k)
    again = _forward(_post(case), k)
    for name in ("boxes", "scores", "labels", "source", "count"):
        assert torch.equal(getattr(det, name), getattr(again, name)), f"{case}: two runs differ in {name}"
    lst = det.to_list()
    for b in range(k["c"]["B"]):
        order = np.argsort(-gold[f"scores{b}"], kind="stable")
        n = len(order)
        assert int(det.count[b]) == n == len(lst[b]["scores"])
        assert np.array_equal(det.source[b, :n].cpu().numpy(), gold[f"source{b}"][order]), f"{case} image {b}: source order"
        assert np.array_equal(lst[b]["labels"].cpu().numpy(), gold[f"labels{b}"][order]), f"{case} image {b}: labels"
        assert bool((det.scores[b, n:] == -1).all()) and bool((det.source[b, n:] == -1).all())
        r64 = k["r64"]
        _check_scores(f"{case} image {b}", det.scores[b, :n], r64["scores"][b, :n])
        _check_boxes(f"{case} image {b}", det.boxes[b, :n], r64["boxes"][b, :n], r64["mag"][b, :n])
        # and against the reference's own fp32 numbers: two fp32 evaluations, each within the bound of the fp64 one
        gb = torch.from_numpy(gold[f"boxes{b}"][order]).to(DEV).double()
        assert bool(((det.boxes[b, :n].double() - gb).abs() <= 2 * dc.box_bound(r64["mag"][b, :n])).all())


def test_abi_refusals(lib):
    k = _case("detect_edge")
    c = k["c"]
    ptr, idx = (t.to(DEV) for t in dc.csr(c["positive_map"], c["C"], True))
    lg, ctr = k["x"]["logits"][0], k["x"]["centerness"][0]
    out = torch.empty((1, 15, 4), device=DEV)
    ok = lambda *a: lib.call("fiber_det_scores_f32", *a)     # noqa: E731
    ok(lib.ptr(lg), lib.ptr(ctr), lib.ptr(ptr), lib.ptr(idx), lib.ptr(out), 1, 15, 256, 4, 0.05, 0)
    ok(None, None, None, None, None, 0, 15, 256, 4, 0.05, 0)                       # B == 0: nothing to do
    for bad in ((lib.ptr(lg), lib.ptr(ctr), lib.ptr(ptr), lib.ptr(idx), lib.ptr(out), 1, 15, 128, 4, 0.05, 0),          # T != 256
                (lib.ptr(lg), lib.ptr(ctr), lib.ptr(ptr), lib.ptr(idx), lib.ptr(out), 1, 15, 256, 0, 0.05, 0),          # C <= 0
                (None, lib.ptr(ctr), lib.ptr(ptr), lib.ptr(idx), lib.ptr(out), 1, 15, 256, 4, 0.05, 0),                 # NULL
                (lib.ptr(lg) + 4, lib.ptr(ctr), lib.ptr(ptr), lib.ptr(idx), lib.ptr(out), 1, 14, 256, 4, 0.05, 0)):     # misaligned
        with pytest.raises(lib.FiberHipError):
            ok(*bad)
    nmax = lib.plain("fiber_det_max_candidates")
    assert nmax >= 15000
    z = torch.zeros(64, device=DEV)
    zi = torch.zeros(64, dtype=torch.int32, device=DEV)
    zl = torch.zeros(64, dtype=torch.int64, device=DEV)
    with pytest.raises(lib.FiberHipError):
        lib.call("fiber_det_nms_mask", lib.ptr(z), lib.ptr(z), lib.ptr(zi), lib.ptr(zl), 1, nmax + 1, 0.5)
    with pytest.raises(lib.FiberHipError):
        lib.call("fiber_det_nms_select", lib.ptr(z), lib.ptr(z), lib.ptr(zi), lib.ptr(zi), lib.ptr(zl), lib.ptr(z), lib.ptr(z), lib.ptr(zi),
                 lib.ptr(zi), lib.ptr(zi), 1, nmax + 1, 10)
    with pytest.raises(lib.FiberHipError):
        lib.call("fiber_det_nms_mask", lib.ptr(z) + 4, lib.ptr(z), lib.ptr(zi), lib.ptr(zl), 1, 4, 0.5)
    with pytest.raises(lib.FiberHipError):                   # the level's slice must lie inside [0, N)
        lib.call("fiber_det_decode_f32", lib.ptr(z), lib.ptr(zl), lib.ptr(z), lib.ptr(z), lib.ptr(z), lib.ptr(z), lib.ptr(z), lib.ptr(zi),
                 lib.ptr(zi), 1, 8, 4, 4, 10, 4, 0, 0.0)
    lib.call("fiber_det_nms_mask", None, None, None, None, 2, 0, 0.5)              # N == 0
    lib.call("fiber_det_nms_select", None, None, None, None, None, None, None, None, None, None, 0, 5, 10)
    torch.cuda.synchronize()


def test_ops_wrappers_take_views(lib):
    from fiber_amd import ops
    k = _case("detect_small")
    c = k["c"]
    ptr, idx = (t.to(DEV) for t in dc.csr(c["positive_map"], c["C"]))
    lg, ctr = k["x"]["logits"][2], k["x"]["centerness"][2]
    want = ops.det_scores(lg, ctr, ptr, idx, c["thresh"], c["agg"])
    wide = torch.zeros((2, 35, 257), device=DEV)
    wide[:, :, 1:] = lg                                      # a view at an odd offset with a row stride of 257
    assert torch.equal(ops.det_scores(wide[:, :, 1:], ctr, ptr, idx, c["thresh"], c["agg"]), want)
    with pytest.raises(NotImplementedError):
        ops.det_scores(lg, ctr, ptr, idx, c["thresh"], "POWER")
    boxes, scores, labels, source = _sorted_candidates(k)
    a = ops.nms_ml(boxes, scores, labels, source, c["nms"], c["D"])
    padded = torch.zeros((2, 600, 5), device=DEV)
    padded[:, :, 1:] = boxes
    b = ops.nms_ml(padded[:, :, 1:], scores, labels.long(), source, c["nms"], c["D"])
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    e = ops.nms_ml(boxes[:, :0], scores[:, :0], labels[:, :0], source[:, :0], c["nms"], 5)
    assert e[0].shape == (2, 5, 4) and int(e[4].sum()) == 0 and bool((e[1] == -1).all())


def _module_cfg():
    cfg = gc.head_cfg(convs=gc.SMALL["convs"])
    d = dc.cfg_for("detect_small")
    for k, v in vars(d.MODEL.RPN).items():
        setattr(cfg.MODEL.RPN, k, v)
    cfg.MODEL.ATSS, cfg.MODEL.DYHEAD.SCORE_AGG, cfg.TEST = d.MODEL.ATSS, "MEAN", d.TEST
    cfg.TEST.MDETR_STYLE_AGGREGATE_CLASS_NUM = 6             # the head has one class channel: the six labels need the v2 mapping's num_class
    return cfg


def test_vldyhead_module_on_ground_small(lib):
    """The head's logits come from bf16 MFMA and the tower from bf16 GEMMs: decisive margins are not guaranteed, so at most 2 % of an
    image's detections may differ as a set from the restatement fed the SAME device tensors (the head's output is captured by a forward
    hook during the module's own call: a second run of the head may round differently); the matched ones meet the float bound."""
    from fiber_amd.modules import VLDyHeadModule
    m = VLDyHeadModule(_module_cfg())
    gc.set_head_weights(m.head)
    m = m.to(DEV).eval()
    assert all(k.startswith("head.") for k in m.state_dict())
    xs, emb, _, _ = gc.small_inputs()
    xs, emb = [x.to(DEV) for x in xs], emb.to(DEV)
    c = dc.CASES["detect_small"]
    pm = c["positive_map"]
    seen = []
    hook = m.head.register_forward_hook(lambda _m, _i, o: seen.append(o))
    det = m([(h, w) for w, h in c["image_sizes"]], xs, {"embedded": emb}, pm)      # forward end to end: the head runs ONCE, here
    hook.remove()
    assert len(seen) == 1
    out = seen[0]                                            # the very tensors the box selector consumed
    sizes = torch.tensor(c["image_sizes"], dtype=torch.float32, device=DEV)
    ref = dc.postprocess_torch(out[6], out[1], out[2], m.anchor_generator(xs), sizes, pm, 6, "MEAN", c["thresh"], c["top_n"], c["nms"], c["D"])
    m.train()
    with pytest.raises(NotImplementedError):
        m([(160, 224)] * 2, xs, {"embedded": emb}, pm)
    for b in range(2):
        n, nr = int(det.count[b]), int(ref["count"][b])
        got, want = det.source[b, :n].tolist(), ref["source"][b, :nr].tolist()
        diff = len(set(got) ^ set(want))
        print(f"image {b}: {n} detections, {nr} in the restatement, {diff} differ as a set")
        assert n > 0 and diff <= 0.02 * max(n, nr), f"image {b}: {diff} of {max(n, nr)} detections differ"
        pos = {s: i for i, s in enumerate(want)}
        gi = [i for i, s in enumerate(got) if s in pos]
        ri = [pos[got[i]] for i in gi]
        _check_scores(f"module image {b}", det.scores[b, gi], ref["scores"][b, ri])
        _check_boxes(f"module image {b}", det.boxes[b, gi], ref["boxes"][b, ri], ref["mag"][b, ri])


def test_postprocessor_in_a_captured_graph(lib):
    k = _case("detect_small")
    post = _post("detect_small")
    fresh = {key: [t.to(DEV) for t in v] for key, v in dc.inputs("detect_small", seed=5).items()}
    static = {key: [t.clone() for t in v] for key, v in k["x"].items()}
    run = lambda x: post(x["bbox_reg"], x["centerness"], k["sizes"], k["anchors"], x["logits"], k["c"]["positive_map"])   # noqa: E731
    want_first, want_fresh = run(k["x"]), run(fresh)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(static)                                          # warm-up on the capture stream: caches, lazy initialisation
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                # a single stream: no parallel branches
        det = run(static)
    g.replay()
    torch.cuda.synchronize()
    for name in ("boxes", "scores", "labels", "source", "count"):
        assert torch.equal(getattr(det, name), getattr(want_first, name)), f"replay differs from eager in {name}"
    for key in static:
        for d, srcc in zip(static[key], fresh[key]):
            d.copy_(srcc)
    g.replay()
    torch.cuda.synchronize()
    for name in ("boxes", "scores", "labels", "source", "count"):
        assert torch.equal(getattr(det, name), getattr(want_fresh, name)), f"replay on fresh inputs differs from eager in {name}"
    assert not torch.equal(want_first.source, want_fresh.source)
