"""CPU tests of COCO-protocol box AP: the CPU path of CocoBoxEvaluator (fiber_amd/modules/detection_eval.py) against the scalar restatement
of tests/coco_eval_cases.py, the hand-worked bits of coco_crowd and coco_cap, the identity with the LVIS protocol where the two coincide
(which ties the path to tables the reference's own LVISEval pinned), the packing and its refusals, make_box_evaluator, synchronize() alone
and on gloo with two ranks, the C ABI.  PARITY UNPINNED against the pycocotools binary (see coco_eval_cases).
Everything is exact: match, ignore, rank, valid and num_gt are integers, and every finite table entry is one fp64 addition and one fp64
division of integers written identically on both sides."""
import os
import re

import numpy as np
import pytest
import torch

import coco_eval_cases as cv
import mp_util

KEYS = ["AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl"]


def _evaluator(k, plus_one, **kw):
    from fiber_amd.modules import CocoBoxEvaluator
    return CocoBoxEvaluator(k["categories"], max_dets=k["max_dets"], plus_one=bool(plus_one), **kw)


def _u64(t):
    return t.numpy().view(np.uint64)


def _same_results(got, want):
    assert list(got) == list(want) and [float(v) for v in got.values()] == [float(v) for v in want.values()], (got, want)


_runs = {}


def _run(case, plus_one):
    """one update on the CPU path, once per (case, plus_one) -> (evaluator, match, ignore, rank, valid)"""
    if (case, plus_one) not in _runs:
        from fiber_amd.modules import pack_coco_targets
        k = cv.case_inputs(case)
        ev = _evaluator(k, plus_one)
        out = ev.update(cv.tensors(k, torch), pack_coco_targets(k["samples"], k["categories"]))
        _runs[case, plus_one] = (ev,) + tuple(out)
    return _runs[case, plus_one]


@pytest.mark.parametrize("case,plus_one", cv.RUNS)
def test_cpu_path_equals_restatement(case, plus_one):
    r = cv.restate(case, plus_one)
    ev, match, ignore, rank, valid = _run(case, plus_one)
    assert np.array_equal(valid.numpy(), r["valid"]) and np.array_equal(rank.numpy(), r["rank"]), f"{case}: valid / rank"
    assert np.array_equal(_u64(match), r["match"]) and np.array_equal(_u64(ignore), r["ignore"]), f"{case}: match / ignore words"
    assert np.array_equal(ev.num_gt.numpy(), r["num_gt"]), f"{case}: num_gt"
    precision, recall = ev.tables()
    assert precision.shape == r["precision"].shape and recall.shape == r["recall"].shape and precision.dtype == torch.float64
    assert np.array_equal(precision.numpy(), r["precision"]) and np.array_equal(recall.numpy(), r["recall"]), f"{case}: tables"
    _same_results(ev.summarize(), r["results"])
    if len(cv.case_inputs(case)["max_dets"]) == 3:
        assert list(ev.results) == KEYS
    assert int((r["match"] != 0).sum()) > 0 and int(r["valid"].sum()) > 0


@pytest.mark.parametrize("case", ["coco_small", "coco_cap"])
def test_two_updates_equal_one(case):
    from fiber_amd.modules import pack_coco_targets
    k = cv.case_inputs(case)
    one = _run(case, 1)[0]
    ev = _evaluator(k, 1)
    B = len(k["samples"])
    G = max(len(s["annotations"]) for s in k["samples"])
    for sl in (slice(0, B // 2), slice(B // 2, B)):
        ev.update(cv.tensors(k, torch, sl), pack_coco_targets(k["samples"][sl], k["categories"], num_boxes=G))
    assert all(torch.equal(a, b) for a, b in zip(ev.tables(), one.tables())) and torch.equal(ev.num_gt, one.num_gt)
    _same_results(ev.summarize(), one.summarize())
    ev.reset()
    assert ev.image_ids == [] and int(ev.num_gt.sum()) == 0
    ev.update(cv.tensors(k, torch), pack_coco_targets(k["samples"], k["categories"]))
    assert all(torch.equal(a, b) for a, b in zip(ev.tables(), one.tables()))
    ev.update(cv.tensors(k, torch, slice(0, 1)), pack_coco_targets(k["samples"][:1], k["categories"]))
    with pytest.raises(ValueError, match="more than once"):
        ev.summarize()


def test_lvis_identity():
    """where the two protocols coincide the COCO path gives the LVIS path's num_gt and tables, bit for bit"""
    from fiber_amd.modules import BoxAPEvaluator, pack_detection_targets
    k = cv.case_inputs("coco_lvis_identity")
    coco = _run("coco_lvis_identity", 0)[0]
    cats, samples = cv.lvis_side()
    lvis = BoxAPEvaluator(cats, max_dets=300)
    _, _, valid = lvis.update(cv.tensors(k, torch), pack_detection_targets(samples, cats))
    d = k["det"]
    held = np.arange(d.labels.shape[1])[None, :] < d.count[:, None]
    assert int(d.count.max()) < 300 and np.array_equal(valid.numpy() != 0, held), "the LVIS side drops or cuts nothing"
    assert np.array_equal(coco.num_gt.numpy(), lvis.num_gt.numpy()) and int(lvis.num_gt.sum()) > 0
    (cp, cr), (lp, lr) = coco.tables(), lvis.tables()
    assert cp.shape == lp.shape + (1,) and cr.shape == lr.shape + (1,)
    assert np.array_equal(cp[..., 0].numpy(), lp.numpy()) and np.array_equal(cr[..., 0].numpy(), lr.numpy())
    got, want = coco.summarize(), lvis.summarize()
    assert [float(got[key]) for key in KEYS[:6]] == [float(want[key]) for key in KEYS[:6]] and float(got["AR300"]) == float(want["AR@300"])


def test_hand_worked_crowd_bits():
    _, match, ignore, rank, valid = _run("coco_crowd", 0)
    ev = _run("coco_crowd", 0)[0]
    count = cv.case_inputs("coco_crowd")["det"].count
    assert sorted(cv.CROWD_BITS) == [(b, d) for b in range(len(count)) for d in range(int(count[b]))]
    for (b, d), (m, ig) in cv.CROWD_BITS.items():
        assert _u64(match)[b, d] == m and _u64(ignore)[b, d] == ig, f"image {b} slot {d}: match {int(_u64(match)[b, d]):#x}, ignore {int(_u64(ignore)[b, d]):#x}"
        assert valid[b, d] == 1
    assert np.array_equal(ev.num_gt.numpy(), cv.CROWD_NUM_GT)
    precision, recall = (t.numpy() for t in ev.tables())
    one_tp = 1.0 / (0.0 + 1.0 + 2.0 ** -52)                  # one true positive and no false one (as false positives: 1 / 3)
    assert (precision[:, :, 0, 0, 2] == one_tp).all() and (recall[:, 0, 0, 2] == 1.0).all(), "(a): the two crowd matches are no false positives"
    assert (precision[:, :, 1] == -1).all(), "(b): a category of crowd ground truth only has no table"
    assert (recall[:3, 2, 0, 2] == 1.0).all() and (recall[3:, 2, 0, 2] == 0.0).all(), "(c): the normal one up to 0.60, the crowd above"
    assert (recall[:, 3, 0, 2] == 1.0).all(), "(d): 'ignore: 1, iscrowd: 0' counts and is matchable"
    assert recall[:, 4, 0, 2].tolist() == [1.0] * 6 + [0.5] * 2 + [0.0] * 2, "(e): the later one of two bit-equal IoUs is taken"
    assert recall[:, 5, 0, 2].tolist() == [1.0] + [0.0] * 9, "(f): IoU exactly 1/2 matches at 0.50"


def test_hand_worked_cap_bits():
    k = cv.case_inputs("coco_cap")
    d = k["det"]
    (ev1, m1, i1, rank, valid), (ev0, m0, i0, rank0, valid0) = _run("coco_cap", 1), _run("coco_cap", 0)
    assert torch.equal(rank, rank0) and torch.equal(valid, valid0)
    five = np.nonzero(d.labels[0, :d.count[0]] == 1)[0]
    nine = np.nonzero(d.labels[0, :d.count[0]] == 2)[0]
    assert len(five) == 103 and len(nine) == 12 and nine[0] < five[-1] and five[0] < nine[-1], "the slot order mixes the labels"
    assert rank[0, five].tolist() == list(range(103)) and rank[0, nine].tolist() == list(range(12))
    assert valid[0, five].tolist() == [1] * 100 + [0] * 3 and valid[0, nine].tolist() == [1] * 12
    assert (rank[0, d.count[0]:] == -1).all() and (valid[0, d.count[0]:] == 0).all()
    cut = five[101]                                          # covers the second ground truth exactly, and does not exist
    assert _u64(m1)[0, cut] == 0 and _u64(i1)[0, cut] == 0 and d.boxes[0, cut].tolist() == [560, 400, 619, 459]
    every = cv.word(cv.EVERY)
    assert _u64(m1)[0, five[0]] == every and (_u64(m1)[0, five[1:]] == 0).all(), "the second ground truth of category 5 stays unmatched"
    assert (_u64(m1)[0, nine] == every).all() and (_u64(m0)[0, nine] == every).all()
    recall = ev1.tables()[1].numpy()                         # [T, C, A, M]
    assert (recall[:, 1, 0, 0] == 1 / 12).all() and (recall[:, 1, 0, 1] == 10 / 12).all() and (recall[:, 1, 0, 2] == 1.0).all()
    res = ev1.summarize()
    assert 0 < res["AR1"] < res["AR10"] < res["AR100"]
    thirteen = int(np.nonzero(d.labels[1, :d.count[1]] == 3)[0][0])
    assert d.boxes[1, thirteen].tolist() == [100, 100, 119, 109.5]
    assert _u64(m1)[1, thirteen] & np.uint64(1) == 1 and _u64(m0)[1, thirteen] & np.uint64(1) == 0, "IoU 0.525 with plus_one, 0.45125 without"


def test_pack_coco_targets_layout_and_refusals():
    from fiber_amd.modules import CocoTargets, pack_coco_targets
    from fiber_amd.modules import detection_eval as de
    k = cv.case_inputs("coco_crowd")
    t = pack_coco_targets(k["samples"], k["categories"], num_boxes=3)
    B = len(k["samples"])
    assert isinstance(t, CocoTargets) and t.gt.shape == (B, 3, 4) and t.gt.dtype == torch.float64 and t.area.dtype == torch.float64
    assert t.category.dtype == torch.int32 and t.crowd.dtype == torch.uint8 and t.gt_count.dtype == torch.int32
    assert t.gt_count.tolist() == [2, 1, 2, 1, 2, 1] and t.image_ids == [10, 11, 12, 13, 14, 15] and t.category_ids == [11, 12, 13, 14, 15, 16]
    assert t.crowd[:, :2].tolist() == [[1, 0], [1, 0], [0, 1], [0, 0], [0, 0], [0, 0]], "'ignore: 1, iscrowd: 0' is not crowd"
    assert t.gt[2, 1].tolist() == [50.0, 50.0, 300.0, 300.0] and t.area[2, 0].item() == 6200.0 and t.category[4].tolist()[:2] == [4, 4]
    assert (t.gt[1, 1:] == 0).all() and t.to("cpu").image_ids == t.image_ids
    cats = k["categories"]
    ann = dict(bbox=[0, 0, 5, 5], area=25.0, category_id=11, iscrowd=0)
    with pytest.raises(ValueError, match="num_boxes"):
        pack_coco_targets(k["samples"], cats, num_boxes=1)
    with pytest.raises(ValueError, match="not in categories"):
        pack_coco_targets([dict(image_id=1, annotations=[dict(ann, category_id=999)])], cats)
    with pytest.raises(ValueError, match="ascending"):
        pack_coco_targets(k["samples"], cats[::-1])
    for box in ([0, 0, 0, 5], [0, 0, 5, -1]):
        with pytest.raises(ValueError, match="no extent"):
            pack_coco_targets([dict(image_id=1, annotations=[dict(ann, bbox=box)])], cats)
    with pytest.raises(ValueError, match="more than once"):
        pack_coco_targets([dict(image_id=1, annotations=[ann]), dict(image_id=1, annotations=[])], cats)
    with pytest.raises(ValueError, match="capacity"):
        pack_coco_targets([dict(image_id=1, annotations=[dict(ann, bbox=[i, 0, 5, 5]) for i in range(de.MAX_GT + 1)])], cats)
    with pytest.raises(ValueError, match="rank counters"):
        pack_coco_targets([], [dict(id=i) for i in range(de.MAX_COCO_CATEGORIES + 1)])


def test_evaluator_refusals_and_names():
    from fiber_amd.modules import BoxAPEvaluator, CocoBoxEvaluator, make_box_evaluator, pack_coco_targets, pack_detection_targets
    k = cv.case_inputs("coco_small")
    cats = k["categories"]
    assert type(make_box_evaluator("coco", cats)) is CocoBoxEvaluator and make_box_evaluator("coco", cats, plus_one=False).plus_one is False
    lvis = make_box_evaluator("lvis", cv.lvis_side()[0], max_dets=50)
    assert type(lvis) is BoxAPEvaluator and lvis.max_dets == 50 and lvis.image_cap == 50
    assert BoxAPEvaluator(cv.lvis_side()[0], fixed_ap_topk=3).image_cap is None and make_box_evaluator("coco", cats).image_cap is None
    assert BoxAPEvaluator.pack_targets is pack_detection_targets and CocoBoxEvaluator.pack_targets is pack_coco_targets
    with pytest.raises(ValueError, match="protocol"):
        make_box_evaluator("voc", cats)
    assert make_box_evaluator("coco", cats).max_dets == (1, 10, 100) and CocoBoxEvaluator.METRICS == tuple(KEYS[:6])
    with pytest.raises(ValueError, match="64 bits"):
        CocoBoxEvaluator(cats, iou_thrs=np.linspace(0.1, 0.9, 17))
    with pytest.raises(ValueError, match="ascend"):
        CocoBoxEvaluator(cats, rec_thrs=[0.5, 0.1])
    for bad in ((), (0, 10), (10, 1), (10, 10)):
        with pytest.raises(ValueError, match="max_dets"):
            CocoBoxEvaluator(cats, max_dets=bad)
    t = pack_coco_targets(k["samples"], cats)
    with pytest.raises(ValueError, match="categories"):
        CocoBoxEvaluator(cats + [dict(id=99)]).update(cv.tensors(k, torch), t)
    with pytest.raises(ValueError, match="samples"):
        CocoBoxEvaluator(cats).update(cv.tensors(k, torch, slice(0, 2)), t)


def test_empty_evaluator_summarises_to_minus_one():
    from fiber_amd.modules import CocoBoxEvaluator, pack_coco_targets
    cats = cv.case_inputs("coco_small")["categories"]
    ev = CocoBoxEvaluator(cats)
    res = ev.summarize()
    assert list(res) == KEYS and all(v == -1 for v in res.values())
    per = ev.per_category()
    assert per["category_ids"] == [c["id"] for c in cats] and all((per[key] == -1).all() for key in ("AP", "AP50", "APs", "APm", "APl"))
    k = cv.case_inputs("coco_small")                          # an update that holds nothing: no ground truth, no detection
    empty = cv.tensors(k, torch, slice(1, 2))
    empty.count = torch.zeros_like(empty.count)
    ev.update(empty, pack_coco_targets([dict(image_id=5, annotations=[])], cats))
    assert all(v == -1 for v in ev.summarize().values())


def test_per_category_rows():
    """summarize_per_category: the PLAIN mean of the category's precision entries at the largest max_dets, -1 entries included"""
    ev = _run("coco_small", 1)[0]
    r = cv.restate("coco_small", 1)
    per = ev.per_category()
    p = r["precision"][..., -1]
    t50 = [t for t in range(cv.T) if cv.IOU_THRS[t] == 0.5]
    for c in range(p.shape[2]):
        assert per["AP"][c] == np.mean(p[:, :, c, 0]) and per["AP50"][c] == np.mean(p[t50][:, :, c, 0])
        assert [per[key][c] for key in ("APs", "APm", "APl")] == [np.mean(p[:, :, c, a]) for a in (1, 2, 3)]
    assert list(per) == ["category_ids", "AP", "AP50", "APs", "APm", "APl"]


def _sync_worker(rank, port, out_dir, case):
    import torch.distributed as dist
    from fiber_amd.modules import pack_coco_targets
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2)
    try:
        k = cv.case_inputs(case)
        B = len(k["samples"])
        sl = slice(0, B // 3) if rank == 0 else slice(B // 3, B)          # unequal shares: the gather pads to the largest
        ev = _evaluator(k, 1)
        ev.update(cv.tensors(k, torch, sl), pack_coco_targets(k["samples"][sl], k["categories"]))
        ev.synchronize()
        precision, recall = ev.tables()
        torch.save((precision, recall, ev.num_gt, ev.summarize(), ev.image_ids), os.path.join(out_dir, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_synchronize_alone_and_on_gloo(tmp_path):
    case = "coco_small"
    one = _run(case, 1)[0]
    before = [t.clone() for t in one.tables()]
    one.synchronize()                                        # no process group: the identity
    assert all(torch.equal(a, b) for a, b in zip(one.tables(), before))
    want = one.summarize()
    mp_util.spawn_with_retry(_sync_worker, lambda port: (port, str(tmp_path), case), nprocs=2, deadline_s=120)
    for r in range(2):
        precision, recall, num_gt, res, ids = torch.load(os.path.join(str(tmp_path), f"r{r}.pt"), weights_only=False)
        assert torch.equal(precision, before[0]) and torch.equal(recall, before[1])
        assert torch.equal(num_gt, one.num_gt) and res == want and sorted(ids) == sorted(one.image_ids)


def test_c_abi_exports_the_coco_entries():
    from fiber_amd import lib, ops
    from fiber_amd.modules import detection_eval as de
    l = lib.load()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fiber_hip.h")).read()
    declared = set(re.findall(r"\b(?:int|long)\s+(fiber_\w+)\s*\(", hdr))
    for name in ("fiber_ap_match_coco", "fiber_ap_coco_max_categories"):
        assert hasattr(l, name) and name in declared and name in lib.exported_symbols(), name
    assert ops.ap_coco_max_categories() == de.MAX_COCO_CATEGORIES >= 1203
