"""GPU tests of COCO-protocol box AP (csrc/apeval.hip: fiber_ap_match_coco, and fiber_ap_accumulate reused per max_dets): the matching
kernel against the package's CPU path and the scalar restatement of tests/coco_eval_cases.py on sentinel-filled outputs with guard words
(every element written, guards intact, two runs bitwise equal); the device tables bit-equal to the host's; updates under sync-debug
"error"; the binding's refusals and the ABI's; evaluate_detection with a CocoBoxEvaluator end to end.  Integers and bits exactly; the
tables with array_equal (every finite entry is one fp64 addition and one correctly rounded fp64 division of integers).
PARITY UNPINNED against the pycocotools binary (see coco_eval_cases)."""
import types

import numpy as np
import pytest
import torch

import coco_eval_cases as cv
import detect_cases as dc
import ground_cases as gc
import ground_eval_cases as ge

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
T, A, R = cv.T, cv.A, len(cv.REC_THRS)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from fiber_amd import lib
    lib.load()
    return lib


def _guarded(n, dtype, fill):
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[:n]


_cases = {}


def _case(case):
    """device tensors and packed targets, once per case"""
    if case not in _cases:
        from fiber_amd.modules import pack_coco_targets
        k = cv.case_inputs(case)
        host_t = pack_coco_targets(k["samples"], k["categories"])
        _cases[case] = dict(k=k, det=cv.tensors(k, torch, device=DEV), host_det=cv.tensors(k, torch), t=host_t.to(DEV), host_t=host_t,
                            thrs=torch.from_numpy(cv.IOU_THRS.copy()).to(DEV), rng=torch.from_numpy(cv.AREA_RNG.copy()).to(DEV))
    return _cases[case]


_host = {}


def _host_run(case, plus_one):
    """the package's CPU path, once per (case, plus_one) -> (evaluator, match, ignore, rank, valid)"""
    if (case, plus_one) not in _host:
        from fiber_amd.modules import CocoBoxEvaluator
        c = _case(case)
        ev = CocoBoxEvaluator(c["k"]["categories"], max_dets=c["k"]["max_dets"], plus_one=bool(plus_one))
        _host[case, plus_one] = (ev,) + tuple(ev.update(c["host_det"], c["host_t"]))
    return _host[case, plus_one]


def _match_args(lib, c, match, ignore, rank, valid, num_gt, plus_one):
    d, t = c["det"], c["t"]
    B, D = d.labels.shape
    return [lib.ptr(d.boxes), lib.ptr(d.labels), lib.ptr(d.count), lib.ptr(t.gt), lib.ptr(t.area), lib.ptr(t.category), lib.ptr(t.crowd),
            lib.ptr(t.gt_count), lib.ptr(c["thrs"]), lib.ptr(c["rng"]), lib.ptr(match), lib.ptr(ignore), lib.ptr(rank), lib.ptr(valid),
            lib.ptr(num_gt), B, D, t.gt.shape[1], len(c["k"]["categories"]), T, A, c["k"]["max_dets"][-1], plus_one]


@pytest.mark.parametrize("case,plus_one", cv.RUNS)
def test_match_kernel_against_host_path_and_restatement(lib, case, plus_one):
    c, r = _case(case), cv.restate(case, plus_one)
    B, D = c["det"].labels.shape
    C = len(c["k"]["categories"])
    n = B * D
    if case == "coco_wide":
        crowd = c["host_t"].crowd[0].numpy()
        assert c["t"].gt.shape[1] > 64 and crowd[64:].sum() == 3 and crowd[:64].sum() == 0, "the crowd regions sit in the second chunk of lanes"
    runs = []
    for base in (0, 1000):                                   # num_gt is added to, not written
        (mb, match), (ib, ignore) = _guarded(n, torch.int64, -77), _guarded(n, torch.int64, -77)
        (rb, rank), (vb, valid), (nb, num_gt) = _guarded(n, torch.int32, -77), _guarded(n, torch.uint8, 99), _guarded(C * A, torch.int64, base)
        lib.call("fiber_ap_match_coco", *_match_args(lib, c, match, ignore, rank, valid, num_gt, plus_one))
        torch.cuda.synchronize()
        for buf, fill, m in ((mb, -77, n), (ib, -77, n), (rb, -77, n), (vb, 99, n), (nb, base, C * A)):
            assert bool((buf[m:] == fill).all()), f"{case}: a guard word was written"
        assert not bool((match == -77).any()) and not bool((ignore == -77).any()) and not bool((rank == -77).any()) and \
            not bool((valid == 99).any()), f"{case}: an element was not written"
        runs.append((match.view(B, D).cpu().numpy().view(np.uint64), ignore.view(B, D).cpu().numpy().view(np.uint64),
                     rank.view(B, D).cpu().numpy(), valid.view(B, D).cpu().numpy(), num_gt.view(C, A).cpu().numpy() - base))
    for a, b in zip(*runs):
        assert np.array_equal(a, b), f"{case}: two runs differ"
    match, ignore, rank, valid, num_gt = runs[0]
    assert np.array_equal(valid, r["valid"]) and np.array_equal(rank, r["rank"]), f"{case}: valid / rank against the restatement"
    assert np.array_equal(match, r["match"]) and np.array_equal(ignore, r["ignore"]), f"{case}: match / ignore against the restatement"
    assert np.array_equal(num_gt, r["num_gt"]), f"{case}: num_gt"
    ev, hm, hi, hr, hv = _host_run(case, plus_one)
    assert np.array_equal(match, hm.numpy().view(np.uint64)) and np.array_equal(ignore, hi.numpy().view(np.uint64)), f"{case}: host path"
    assert np.array_equal(rank, hr.numpy()) and np.array_equal(valid, hv.numpy()) and np.array_equal(num_gt, ev.num_gt.numpy())
    if case == "coco_crowd":
        for (b, d), (m, ig) in cv.CROWD_BITS.items():
            assert match[b, d] == m and ignore[b, d] == ig, f"image {b} slot {d}"


@pytest.mark.parametrize("case,plus_one", cv.RUNS)
def test_device_tables_equal_host_tables(lib, case, plus_one):
    """the evaluator on the device, fed as two updates without a synchronisation: tables bit-equal to the host path's and the restatement's"""
    from fiber_amd.modules import CocoBoxEvaluator, pack_coco_targets
    c, r = _case(case), cv.restate(case, plus_one)
    k, det = c["k"], c["det"]
    B = det.labels.shape[0]
    G = c["t"].gt.shape[1]
    parts = [slice(0, B // 2), slice(B // 2, B)]
    fed = [(types.SimpleNamespace(boxes=det.boxes[sl], scores=det.scores[sl], labels=det.labels[sl], count=det.count[sl]),
            pack_coco_targets(k["samples"][sl], k["categories"], num_boxes=G).to(DEV)) for sl in parts]
    ev = CocoBoxEvaluator(k["categories"], max_dets=k["max_dets"], plus_one=bool(plus_one))
    ev.update(det, c["t"])                                   # the one update that allocates the evaluator's device state
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
    host = _host_run(case, plus_one)[0]
    hp, hr = (t.numpy() for t in host.tables())
    precision, recall = precision.cpu().numpy(), recall.cpu().numpy()
    for name, got, want in (("precision", precision, hp), ("recall", recall, hr)):
        bad = got != want
        print(f"{case}: {name} entries differing from the host path: {int(bad.sum())}" + (f", by up to {np.abs(got - want)[bad].max():.3e}" if bad.any() else ""))
    assert np.array_equal(ev.num_gt.cpu().numpy(), r["num_gt"])
    assert np.array_equal(precision, hp) and np.array_equal(recall, hr), f"{case}: host path"
    assert np.array_equal(precision, r["precision"]) and np.array_equal(recall, r["recall"]), f"{case}: restatement"
    got = ev.summarize()
    assert list(got) == list(r["results"]) and [float(v) for v in got.values()] == [float(v) for v in r["results"].values()]
    if case == "coco_wide":
        from fiber_amd import ops
        kept = int((cv.restate(case, plus_one)["valid"] != 0).sum())
        assert kept > 3 * ops.ap_chunk(), "a category spans more than three chunks of the accumulation's scans"


def test_lvis_identity_on_the_device(lib):
    from fiber_amd.modules import BoxAPEvaluator, CocoBoxEvaluator, pack_detection_targets
    c = _case("coco_lvis_identity")
    cats, samples = cv.lvis_side()
    coco = CocoBoxEvaluator(c["k"]["categories"], max_dets=(300,), plus_one=False)
    coco.update(c["det"], c["t"])
    lvis = BoxAPEvaluator(cats, max_dets=300)
    lvis.update(c["det"], pack_detection_targets(samples, cats).to(DEV))
    (cp, cr), (lp, lr) = coco.tables(), lvis.tables()
    assert torch.equal(coco.num_gt, lvis.num_gt) and torch.equal(cp[..., 0], lp) and torch.equal(cr[..., 0], lr)


def test_binding_refusals_launch_nothing(lib):
    from fiber_amd import ops
    c = _case("coco_small")
    d, t = c["det"], c["t"]
    B, D = d.labels.shape
    C, G = len(c["k"]["categories"]), t.gt.shape[1]

    def call(num_gt, thrs=c["thrs"], rng=c["rng"], gt=t):
        return ops.ap_match_coco(d.boxes, d.labels, d.count, gt.gt, gt.area, gt.category, gt.crowd, gt.gt_count, thrs, rng, num_gt, 100, True)
    num_gt = torch.zeros((C, A), dtype=torch.int64, device=DEV)
    match, ignore, rank, valid = call(num_gt)
    r = cv.restate("coco_small", 1)
    assert np.array_equal(match.cpu().numpy().view(np.uint64), r["match"]) and np.array_equal(rank.cpu().numpy(), r["rank"])
    assert np.array_equal(num_gt.cpu().numpy(), r["num_gt"]) and match.dtype == torch.int64 and rank.dtype == torch.int32 and valid.dtype == torch.uint8
    wide = torch.zeros((C, 7), dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="64 bits"):         # T * A = 70
        call(wide, rng=torch.tensor([[0.0, 1e10]] * 7, dtype=torch.float64, device=DEV))
    G2 = ops.ap_max_gt() + 1
    big = types.SimpleNamespace(gt=torch.zeros((B, G2, 4), dtype=torch.float64, device=DEV), area=torch.zeros((B, G2), dtype=torch.float64, device=DEV),
                                category=torch.zeros((B, G2), dtype=torch.int32, device=DEV), crowd=torch.zeros((B, G2), dtype=torch.uint8, device=DEV),
                                gt_count=t.gt_count)
    with pytest.raises(ValueError, match="capacity"):
        call(torch.zeros((C, A), dtype=torch.int64, device=DEV), gt=big)
    many = torch.zeros((ops.ap_coco_max_categories() + 1, A), dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="rank counters"):
        call(many)
    with pytest.raises(ValueError, match="uint8"):
        call(torch.zeros((C, A), dtype=torch.int64, device=DEV), gt=types.SimpleNamespace(gt=t.gt, area=t.area, category=t.category,
                                                                                       crowd=t.crowd.to(torch.int32), gt_count=t.gt_count))
    torch.cuda.synchronize()
    assert int(wide.sum()) == 0 and int(many.sum()) == 0, "a refused call adds nothing to num_gt"


def test_match_abi_refusals(lib):
    c = _case("coco_small")
    d, t = c["det"], c["t"]
    B, D = d.labels.shape
    C = len(c["k"]["categories"])
    match, ignore = torch.zeros(B * D, dtype=torch.int64, device=DEV), torch.zeros(B * D, dtype=torch.int64, device=DEV)
    rank, valid = torch.zeros(B * D, dtype=torch.int32, device=DEV), torch.zeros(B * D, dtype=torch.uint8, device=DEV)
    num_gt = torch.zeros((C, 7), dtype=torch.int64, device=DEV)
    thrs = torch.linspace(0.1, 0.9, 17, dtype=torch.float64, device=DEV)
    rng = torch.tensor([[0.0, 1e10]] * 7, dtype=torch.float64, device=DEV)
    good = _match_args(lib, c, match, ignore, rank, valid, num_gt, 1)
    lib.call("fiber_ap_match_coco", *good)
    pos = dict(boxes=0, labels=1, count=2, gt=3, crowd=6, thrs=8, rng=9, match=10, rank=12, valid=13, num_gt=14, B=15, D=16, G=17, C=18, T=19, A=20,
               cap=21, plus_one=22)

    def call(**over):
        args = list(good)
        args[pos["thrs"]], args[pos["rng"]] = lib.ptr(thrs), lib.ptr(rng)
        for name, v in over.items():
            args[pos[name]] = v
        lib.call("fiber_ap_match_coco", *args)
    call(T=16, A=4)                                          # 64 bits: the most a word holds
    call(T=9, A=7, plus_one=0, cap=0)
    for bad in (dict(T=17, A=4), dict(T=10, A=7), dict(T=0), dict(A=0), dict(C=0), dict(B=-1), dict(D=-1), dict(G=-1), dict(cap=-1),
                dict(plus_one=2), dict(plus_one=-1), dict(G=int(lib.plain("fiber_ap_max_gt")) + 1),
                dict(C=int(lib.plain("fiber_ap_coco_max_categories")) + 1), dict(boxes=None), dict(labels=None), dict(count=None), dict(gt=None),
                dict(crowd=None), dict(thrs=None), dict(rng=None), dict(match=None), dict(rank=None), dict(valid=None), dict(num_gt=None),
                dict(boxes=lib.ptr(d.boxes) + 4), dict(gt=lib.ptr(t.gt) + 4), dict(labels=lib.ptr(d.labels) + 2), dict(rank=lib.ptr(rank) + 2)):
        with pytest.raises(lib.FiberHipError):
            call(**bad)
    before = num_gt.clone()
    call(B=0, boxes=None, labels=None, count=None, gt=None, match=None, rank=None, num_gt=None)      # B == 0: no launch, nothing read
    torch.cuda.synchronize()
    assert torch.equal(before, num_gt) and int(lib.plain("fiber_ap_coco_max_categories")) >= 1203


def _module_cfg():
    cfg = gc.head_cfg(convs=gc.SMALL["convs"])
    d = dc.cfg_for("detect_small")
    for k, v in vars(d.MODEL.RPN).items():
        setattr(cfg.MODEL.RPN, k, v)
    cfg.MODEL.ATSS, cfg.MODEL.DYHEAD.SCORE_AGG, cfg.TEST = d.MODEL.ATSS, "MEAN", d.TEST
    cfg.TEST.MDETR_STYLE_AGGREGATE_CLASS_NUM = ge.MAPS_C
    return cfg


class _TinyDetector(torch.nn.Module):
    """VLDyHeadModule on fixed features behind the call evaluate_detection makes"""

    def __init__(self, head, features):
        super().__init__()
        self.head, self.features = head, features

    def forward(self, images, tokenizer_input=None, positive_map=None):
        self.last = self.head(images.image_sizes, self.features, {"embedded": tokenizer_input}, positive_map)
        return self.last


def test_evaluate_detection_with_the_coco_evaluator(lib):
    """VLDyHeadModule on the ground_small weights -> evaluate_detection -> CocoBoxEvaluator on the device: equal to the host evaluator fed
    the same Detections, with ground truth made of the image's own detections (every ninth one crowd) so that some match."""
    from fiber_amd.data import DetImageList
    from fiber_amd.modules import VLDyHeadModule, evaluate_detection, make_box_evaluator
    m = VLDyHeadModule(_module_cfg())
    gc.set_head_weights(m.head)
    xs, emb, _, _ = gc.small_inputs()
    xs, emb = [ge.three(x).to(DEV) for x in xs], ge.three(emb).to(DEV)
    model = _TinyDetector(m.to(DEV).eval(), xs)
    sizes = [(160, 224), (150, 200), (160, 224)]
    images = DetImageList(None, sizes, [(480, 672, 0), (375, 500, 0), (240, 336, 0)])
    with torch.no_grad():
        det = model(images, tokenizer_input=emb, positive_map=ge.MAPS)
    boxes = images.boxes_to_original(det)
    hb, hl, hc = boxes.cpu().numpy(), det.labels.cpu().numpy(), det.count.cpu().numpy()
    assert (hc > 0).all()
    cats = [dict(id=10 * (i + 1)) for i in range(ge.MAPS_C)]
    samples = []
    for b in range(3):
        anns = []
        for i in range(0, int(hc[b]), 3):                    # every third detection, grown by a pixel, is a ground truth of its class
            x1, y1, x2, y2 = [float(v) for v in hb[b, i]]
            if x2 - x1 > 1 and y2 - y1 > 1:
                w, h = float(np.ceil(x2 - x1)) + 1, float(np.ceil(y2 - y1)) + 1
                anns.append(dict(bbox=[float(np.floor(x1)), float(np.floor(y1)), w, h], area=w * h, category_id=cats[int(hl[b, i]) - 1]["id"],
                                 iscrowd=1 if i % 9 == 0 else 0))
        samples.append(dict(image_id=b, annotations=anns[:64]))
    ev = make_box_evaluator("coco", cats)
    targets = ev.pack_targets(samples, cats)
    got = evaluate_detection(model, [dict(images=images, tokenizer_input=emb, positive_maps=ge.MAPS, targets=targets)], ev)
    host = make_box_evaluator("coco", cats)
    det = model.last                                         # the Detections the evaluator was given
    host_det = types.SimpleNamespace(boxes=det.boxes.cpu(), scores=det.scores.cpu(), labels=det.labels.cpu(), count=det.count.cpu())
    hm, hi, hr, hv = host.update(host_det, targets, boxes=images.boxes_to_original(det).cpu())
    _, _, dm, di, dv_, dr = ev._gathered()
    assert torch.equal(dm.cpu(), hm.reshape(-1)) and torch.equal(di.cpu(), hi.reshape(-1)) and torch.equal(dr.cpu(), hr.reshape(-1))
    assert torch.equal(dv_.cpu(), hv.reshape(-1)) and torch.equal(ev.num_gt.cpu(), host.num_gt)
    assert int((hm != 0).sum()) > 0 and int((hm & hi != 0).sum()) > 0 and int(hv.sum()) > 0, "some match, some of them a crowd region"
    (dp, drc), (hp, hrc) = ev.tables(), host.tables()
    assert np.array_equal(dp.cpu().numpy(), hp.numpy()) and np.array_equal(drc.cpu().numpy(), hrc.numpy())
    want = host.summarize()
    assert list(got) == list(want) and [float(v) for v in got.values()] == [float(v) for v in want.values()]
    assert got["AP"] > 0 and got["AR100"] >= got["AR10"] >= got["AR1"] > 0
