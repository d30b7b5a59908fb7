"""GPU tests of box AP evaluation (csrc/apeval.hip): the matching kernel and the accumulation kernel against the reference-run fixtures
tests/golden/apeval_*.npz and the scalar restatement of tests/det_eval_cases.py, on sentinel / NaN-filled outputs with guard words (every
element written, guards intact, two runs bitwise equal); accumulation over updates; update under sync-debug "error"; ABI refusals;
VLDyHeadModule -> boxes_to_original -> BoxAPEvaluator end to end.  Integers exactly; the tables bit-equal (every finite entry is one
fp64 addition and one correctly rounded fp64 division of integers)."""
import types

import numpy as np
import pytest
import torch

import det_eval_cases as dv
import detect_cases as dc
import ground_cases as gc
import ground_eval_cases as ge

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
NAN = float("nan")
ALL = list(dv.CASES)
T, A, R = len(dv.IOU_THRS), len(dv.AREA_RNG), len(dv.REC_THRS)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from fiber_amd import lib
    lib.load()
    return lib


def _guarded(n, dtype, fill):
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[:n]


def _guard_intact(buf, n, fill):
    tail = buf[n:]
    return bool(torch.isnan(tail).all()) if fill != fill else bool((tail == fill).all())


_cases = {}


def _case(case):
    """device tensors, packed targets and the restatement, once per case"""
    if case not in _cases:
        from fiber_amd.modules import pack_detection_targets
        k = dv.case_inputs(case)
        d = k["det"]
        det = types.SimpleNamespace(boxes=torch.from_numpy(d.boxes).to(DEV), scores=torch.from_numpy(d.scores).to(DEV),
                                    labels=torch.from_numpy(d.labels).to(DEV), count=torch.from_numpy(d.count).to(DEV))
        _cases[case] = dict(k=k, det=det, t=pack_detection_targets(k["samples"], k["categories"]).to(DEV), r=dv.restate(case),
                            max_dets=-1 if k["topk"] is not None else k["max_dets"],
                            thrs=torch.from_numpy(dv.IOU_THRS.copy()).to(DEV), rng=torch.from_numpy(dv.AREA_RNG.copy()).to(DEV),
                            rec=torch.from_numpy(dv.REC_THRS.copy()).to(DEV))
    return _cases[case]


def _match_args(lib, c, match, ignore, valid, num_gt):
    d, t = c["det"], c["t"]
    B, D = d.labels.shape
    return [lib.ptr(d.boxes), lib.ptr(d.labels), lib.ptr(d.count), lib.ptr(t.gt), lib.ptr(t.area), lib.ptr(t.category), lib.ptr(t.ignore),
            lib.ptr(t.gt_count), lib.ptr(t.neg_mask), lib.ptr(t.nel_mask), lib.ptr(c["thrs"]), lib.ptr(c["rng"]), lib.ptr(match), lib.ptr(ignore),
            lib.ptr(valid), lib.ptr(num_gt), B, D, t.gt.shape[1], len(c["k"]["categories"]), T, A, c["max_dets"]]


@pytest.mark.parametrize("case", ALL)
def test_match_kernel_against_fixture_and_restatement(lib, golden, case):
    gold, c = golden(case), _case(case)
    B, D = c["det"].labels.shape
    C = len(c["k"]["categories"])
    n = B * D
    runs = []
    for base in (0, 1000):                                   # num_gt is added to, not written
        (mb, match), (ib, ignore) = _guarded(n, torch.int64, -77), _guarded(n, torch.int64, -77)
        (vb, valid), (nb, num_gt) = _guarded(n, torch.uint8, 99), _guarded(C * A, torch.int64, base)
        lib.call("fiber_ap_match", *_match_args(lib, c, match, ignore, valid, num_gt))
        torch.cuda.synchronize()
        assert _guard_intact(mb, n, -77) and _guard_intact(ib, n, -77) and _guard_intact(vb, n, 99) and _guard_intact(nb, C * A, base)
        assert not bool((match == -77).any()) and not bool((ignore == -77).any()) and not bool((valid == 99).any()), f"{case}: an element was not written"
        runs.append((match.view(B, D).cpu().numpy().view(np.uint64), ignore.view(B, D).cpu().numpy().view(np.uint64), valid.view(B, D).cpu().numpy(),
                     num_gt.view(C, A).cpu().numpy() - base))
    for a, b in zip(*runs):
        assert np.array_equal(a, b), f"{case}: two runs differ"
    match, ignore, valid, num_gt = runs[0]
    r = c["r"]
    assert np.array_equal(valid, r["valid"]) and np.array_equal(match, r["match"]) and np.array_equal(ignore, r["ignore"]), f"{case}: restatement"
    assert np.array_equal(num_gt, r["num_gt"]) and np.array_equal(num_gt, gold["num_gt"]), f"{case}: num_gt"
    kept = gold["kept"] == 1
    assert (valid[kept] == 1).all() and np.array_equal(match[kept], gold["match"][kept]) and np.array_equal(ignore[kept], gold["ignore"][kept])
    if c["k"]["topk"] is None:
        assert np.array_equal(valid, gold["kept"]) and np.array_equal(match, gold["match"]) and np.array_equal(ignore, gold["ignore"])


@pytest.mark.parametrize("case", ALL)
def test_accumulate_kernel_against_fixture_and_restatement(lib, golden, case):
    gold, c = golden(case), _case(case)
    r = c["r"]
    C = len(c["k"]["categories"])
    flat, seg = dv.ordered_records(r["records"])
    chunk = int(lib.plain("fiber_ap_chunk"))
    if case == "apeval_wide":
        assert int(np.diff(seg).max()) >= 3 * chunk, "a category spans at least three chunks of the scans"
    rows = (np.array([b for b, _ in flat], np.int64), np.array([d for _, d in flat], np.int64))
    match = torch.from_numpy(r["match"][rows].view(np.int64).copy()).to(DEV)
    ignore = torch.from_numpy(r["ignore"][rows].view(np.int64).copy()).to(DEV)
    seg_ptr, num_gt = torch.from_numpy(seg).to(DEV), torch.from_numpy(r["num_gt"].copy()).to(DEV)
    runs = []
    for _ in range(2):
        (pb, precision), (rb, recall) = _guarded(T * R * C * A, torch.float64, NAN), _guarded(T * C * A, torch.float64, NAN)
        lib.call("fiber_ap_accumulate", lib.ptr(match), lib.ptr(ignore), lib.ptr(seg_ptr), lib.ptr(num_gt), lib.ptr(c["rec"]), lib.ptr(precision),
                 lib.ptr(recall), len(flat), C, T, A, R)
        torch.cuda.synchronize()
        assert _guard_intact(pb, T * R * C * A, NAN) and _guard_intact(rb, T * C * A, NAN)
        assert not bool(torch.isnan(precision).any()) and not bool(torch.isnan(recall).any()), f"{case}: an element was not written"
        runs.append((precision.view(T, R, C, A).cpu().numpy(), recall.view(T, C, A).cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), f"{case}: two runs differ"
    for name, got, want in (("precision", runs[0][0], gold["precision"]), ("recall", runs[0][1], gold["recall"])):
        bad = got != want
        print(f"{case}: {name} entries differing from the reference: {int(bad.sum())}" + (f", by up to {np.abs(got - want)[bad].max():.3e}" if bad.any() else ""))
    assert np.array_equal(runs[0][0], r["precision"]) and np.array_equal(runs[0][1], r["recall"]), f"{case}: restatement"
    assert np.array_equal(runs[0][0], gold["precision"]) and np.array_equal(runs[0][1], gold["recall"]), f"{case}: reference"


def test_accumulate_without_records(lib):
    """ground truth and no record: precision 0 and recall 0; no ground truth: both -1"""
    C = 3
    num_gt = torch.tensor([[2, 0, 2, 0], [0, 0, 0, 0], [1, 1, 0, 0]], dtype=torch.int64, device=DEV)
    seg_ptr = torch.zeros(C + 1, dtype=torch.int64, device=DEV)
    rec = torch.from_numpy(dv.REC_THRS.copy()).to(DEV)
    precision, recall = torch.full((T, R, C, A), NAN, dtype=torch.float64, device=DEV), torch.full((T, C, A), NAN, dtype=torch.float64, device=DEV)
    lib.call("fiber_ap_accumulate", None, None, lib.ptr(seg_ptr), lib.ptr(num_gt), lib.ptr(rec), lib.ptr(precision), lib.ptr(recall), 0, C, T, A, R)
    torch.cuda.synchronize()
    want = torch.where(num_gt > 0, 0.0, -1.0).to(torch.float64)
    assert torch.equal(recall, want.expand(T, C, A)) and torch.equal(precision, want.expand(T, R, C, A))


@pytest.mark.parametrize("case", ALL)
def test_evaluator_accumulates_over_updates_without_synchronising(lib, golden, case):
    from fiber_amd.modules import BoxAPEvaluator, pack_detection_targets
    gold, c = golden(case), _case(case)
    k, det = c["k"], c["det"]
    B = det.labels.shape[0]
    G = c["t"].gt.shape[1]
    parts = [slice(0, B)] if B < 2 else [slice(0, B // 2), slice(B // 2, B)]
    fed = [(types.SimpleNamespace(boxes=det.boxes[sl], scores=det.scores[sl], labels=det.labels[sl], count=det.count[sl]),
            pack_detection_targets(k["samples"][sl], k["categories"], num_boxes=G).to(DEV)) for sl in parts]
    ev = BoxAPEvaluator(k["categories"], max_dets=k["max_dets"], fixed_ap_topk=k["topk"])
    ev.update(c["det"], c["t"])                              # the one update that allocates the evaluator's device state
    one = [t.clone() for t in ev.tables()]
    ev.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for d, t in fed:
            ev.update(d, t)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    precision, recall = ev.tables()
    assert torch.equal(precision, one[0]) and torch.equal(recall, one[1]), f"{case}: two updates differ from one"
    assert np.array_equal(ev.num_gt.cpu().numpy(), gold["num_gt"])
    assert np.array_equal(precision.cpu().numpy(), gold["precision"]) and np.array_equal(recall.cpu().numpy(), gold["recall"]), f"{case}: tables"
    got = ev.summarize()
    assert list(got) == gold["results_keys"].tolist() and [float(v) for v in got.values()] == gold["results_vals"].tolist()
    ev.update(*fed[0])
    with pytest.raises(ValueError, match="more than once"):
        ev.summarize()


def test_match_abi_refusals(lib):
    c = _case("apeval_small")
    d, t = c["det"], c["t"]
    B, D = d.labels.shape
    C, G = len(c["k"]["categories"]), t.gt.shape[1]
    match, ignore = torch.zeros(B * D, dtype=torch.int64, device=DEV), torch.zeros(B * D, dtype=torch.int64, device=DEV)
    valid, num_gt = torch.zeros(B * D, dtype=torch.uint8, device=DEV), torch.zeros((C, 7), dtype=torch.int64, device=DEV)
    thrs = torch.linspace(0.1, 0.9, 17, dtype=torch.float64, device=DEV)
    rng = torch.tensor([[0.0, 1e10]] * 7, dtype=torch.float64, device=DEV)
    good = _match_args(lib, c, match, ignore, valid, num_gt)
    lib.call("fiber_ap_match", *good)
    pos = dict(boxes=0, labels=1, count=2, gt=3, thrs=10, rng=11, match=12, num_gt=15, B=16, D=17, G=18, C=19, T=20, A=21)

    def call(**over):
        args = list(good)
        args[pos["thrs"]], args[pos["rng"]] = lib.ptr(thrs), lib.ptr(rng)
        for name, v in over.items():
            args[pos[name]] = v
        lib.call("fiber_ap_match", *args)
    call(T=16, A=4)                                          # 64 bits: the most a word holds
    call(T=9, A=7)
    for bad in (dict(T=17, A=4), dict(T=10, A=7), dict(T=0), dict(A=0), dict(C=0), dict(B=-1), dict(D=-1), dict(G=-1),
                dict(G=int(lib.plain("fiber_ap_max_gt")) + 1), dict(boxes=None), dict(labels=None), dict(count=None), dict(gt=None), dict(thrs=None),
                dict(rng=None), dict(match=None), dict(num_gt=None), dict(boxes=lib.ptr(d.boxes) + 4), dict(gt=lib.ptr(t.gt) + 4),
                dict(labels=lib.ptr(d.labels) + 2)):
        with pytest.raises(lib.FiberHipError):
            call(**bad)
    before = num_gt.clone()
    call(B=0, boxes=None, labels=None, count=None, gt=None, match=None, num_gt=None)      # B == 0: no launch, nothing read
    torch.cuda.synchronize()
    assert torch.equal(before, num_gt) and int(lib.plain("fiber_ap_max_gt")) >= 1024

    seg_ptr, rec = torch.zeros(C + 1, dtype=torch.int64, device=DEV), c["rec"]
    precision, recall = torch.zeros(17 * R * C * 7, dtype=torch.float64, device=DEV), torch.zeros(17 * C * 7, dtype=torch.float64, device=DEV)
    ngt = torch.zeros((C, 7), dtype=torch.int64, device=DEV)

    def acc(match=lib.ptr(match), seg=lib.ptr(seg_ptr), ngt_=lib.ptr(ngt), prec=lib.ptr(precision), rcl=lib.ptr(recall), N=0, C_=C, T_=T, A_=A, R_=R):
        lib.call("fiber_ap_accumulate", match, lib.ptr(ignore), seg, ngt_, lib.ptr(rec), prec, rcl, N, C_, T_, A_, R_)
    acc()
    acc(T_=16, A_=4)
    for bad in (dict(T_=17, A_=4), dict(T_=0), dict(A_=0), dict(C_=0), dict(N=-1), dict(R_=-1), dict(seg=None), dict(ngt_=None), dict(prec=None),
                dict(rcl=None), dict(match=None, N=5), dict(prec=lib.ptr(precision) + 4)):
        with pytest.raises(lib.FiberHipError):
            acc(**bad)
    torch.cuda.synchronize()


def _module_cfg():
    cfg = gc.head_cfg(convs=gc.SMALL["convs"])
    d = dc.cfg_for("detect_small")
    for k, v in vars(d.MODEL.RPN).items():
        setattr(cfg.MODEL.RPN, k, v)
    cfg.MODEL.ATSS, cfg.MODEL.DYHEAD.SCORE_AGG, cfg.TEST = d.MODEL.ATSS, "MEAN", d.TEST
    cfg.TEST.MDETR_STYLE_AGGREGATE_CLASS_NUM = ge.MAPS_C
    return cfg


def test_module_to_evaluator_end_to_end(lib):
    """VLDyHeadModule on the ground_small weights, boxes_to_original, BoxAPEvaluator: equal to the restatement run on those same detections
    (copied to the host), with ground truth made of the image's own detections so that some match."""
    from fiber_amd.data import DetImageList
    from fiber_amd.modules import BoxAPEvaluator, VLDyHeadModule, pack_detection_targets
    m = VLDyHeadModule(_module_cfg())
    gc.set_head_weights(m.head)
    m = m.to(DEV).eval()
    xs, emb, _, _ = gc.small_inputs()
    xs, emb = [ge.three(x).to(DEV) for x in xs], ge.three(emb).to(DEV)
    sizes = [(160, 224), (150, 200), (160, 224)]
    images = DetImageList(None, sizes, [(480, 672, 0), (375, 500, 0), (240, 336, 0)])
    det = m(sizes, xs, {"embedded": emb}, ge.MAPS)
    boxes = images.boxes_to_original(det)
    hb, hs, hl, hc = boxes.cpu().numpy(), det.scores.cpu().numpy(), det.labels.cpu().numpy(), det.count.cpu().numpy()
    assert (hc > 0).all()
    cats = [dict(id=10 * (i + 1), frequency="rcf"[i % 3]) for i in range(ge.MAPS_C)]
    samples = []
    for b in range(3):
        anns = []
        for i in range(0, int(hc[b]), 3):                    # every third detection, grown by a pixel, is a ground truth of its class
            x1, y1, x2, y2 = [float(v) for v in hb[b, i]]
            if x2 - x1 > 1 and y2 - y1 > 1:
                w, h = float(np.ceil(x2 - x1)) + 1, float(np.ceil(y2 - y1)) + 1
                anns.append(dict(bbox=[float(np.floor(x1)), float(np.floor(y1)), w, h], area=w * h, category_id=cats[int(hl[b, i]) - 1]["id"]))
        present = {a["category_id"] for a in anns}
        samples.append(dict(image_id=b, annotations=anns[:64], neg_category_ids=[c["id"] for c in cats[:2] if c["id"] not in present],
                            not_exhaustive_category_ids=[]))
    ev = BoxAPEvaluator(cats, max_dets=50)
    match, ignore, valid = ev.update(det, pack_detection_targets(samples, cats).to(DEV), boxes=boxes)
    k = dict(categories=cats, samples=samples, max_dets=50, topk=None, det=types.SimpleNamespace(boxes=hb, scores=hs, labels=hl, count=hc))
    r = dv.restate_match(k)
    assert np.array_equal(match.cpu().numpy().view(np.uint64), r["match"]) and np.array_equal(ignore.cpu().numpy().view(np.uint64), r["ignore"])
    assert np.array_equal(valid.cpu().numpy(), r["valid"]) and np.array_equal(ev.num_gt.cpu().numpy(), r["num_gt"])
    assert int((r["match"] != 0).sum()) > 0 and int(r["valid"].sum()) > 0
    got = ev.summarize()
    records = dv.kept_records(k, r["valid"])                 # (equal scores rank in arrival order in both)
    precision, recall = dv.restate_accumulate(records, r["match"], r["ignore"], r["num_gt"], T)
    tp, tr = ev.tables()
    assert np.array_equal(tp.cpu().numpy(), precision) and np.array_equal(tr.cpu().numpy(), recall)
    assert [float(v) for v in got.values()] == [float(v) for v in dv.restate_results(k, precision, recall).values()]
    assert got["AP"] > 0 and "AR@50" in got
