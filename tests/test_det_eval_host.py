"""CPU tests of box AP evaluation: the scalar restatement of tests/det_eval_cases.py and the CPU path of BoxAPEvaluator
(fiber_amd/modules/detection_eval.py) against tests/golden/apeval_*.npz, which the reference's own LVISEval / LvisEvaluatorFixedAP produced
(tools/gen_det_eval_golden.py); the packing of detection targets; refusals; synchronize() on gloo with two ranks; the C ABI.
Everything is exact: match, ignore, valid and num_gt are integers, and every finite table entry is one fp64 addition and one fp64 division
of integers, so the tables and the summary must be bit-equal to the fixture."""
import os
import re
import types

import numpy as np
import pytest
import torch

import det_eval_cases as dv
import mp_util

ALL = list(dv.CASES)


def _tensors(k, sl=slice(None)):
    d = k["det"]
    return types.SimpleNamespace(boxes=torch.from_numpy(d.boxes[sl]), scores=torch.from_numpy(d.scores[sl]), labels=torch.from_numpy(d.labels[sl]),
                                 count=torch.from_numpy(d.count[sl]))


def _evaluator(k, **kw):
    from fiber_amd.modules import BoxAPEvaluator
    return BoxAPEvaluator(k["categories"], max_dets=k["max_dets"], fixed_ap_topk=k["topk"], **kw)


def _results_of(gold):
    return dict(zip(gold["results_keys"].tolist(), gold["results_vals"].tolist()))


def _same_tables(case, what, precision, recall, gold):
    for name, got in (("precision", precision), ("recall", recall)):
        got = np.asarray(got)
        assert got.shape == gold[name].shape and got.dtype == np.float64
        bad = got != gold[name]
        assert not bad.any(), f"{case}: {what} {name} differs from the reference in {int(bad.sum())} entries, by up to {np.abs(got - gold[name])[bad].max():.3e}"


def _same_slots(case, what, match, ignore, valid, gold, k):
    kept = gold["kept"] == 1
    if k["topk"] is None:                                    # the reference evaluated exactly the valid slots
        assert np.array_equal(valid, gold["kept"]), f"{case}: {what} valid"
        assert np.array_equal(match, gold["match"]) and np.array_equal(ignore, gold["ignore"]), f"{case}: {what} match / ignore words"
    else:                                                    # the reference matched after truncating; its records are a subset
        assert (valid[kept] == 1).all()
        assert np.array_equal(match[kept], gold["match"][kept]) and np.array_equal(ignore[kept], gold["ignore"][kept]), f"{case}: {what} match / ignore words"


def test_fixture_margins(golden):
    for case in ALL:
        gold = golden(case)
        assert float(gold["margin_iou"]) >= dv.MARGIN
        assert gold["precision"].nbytes < (1 << 20)


@pytest.mark.parametrize("case", ALL)
def test_restatement_reproduces_fixture(golden, case):
    gold, k, r = golden(case), dv.case_inputs(case), dv.restate(case)
    _same_slots(case, "restatement", r["match"], r["ignore"], r["valid"], gold, k)
    assert np.array_equal(r["num_gt"], gold["num_gt"])
    kept = np.zeros_like(gold["kept"])
    for rows in r["records"]:
        for slot in rows:
            kept[slot] = 1
    assert np.array_equal(kept, gold["kept"]), f"{case}: the kept records"
    _same_tables(case, "restatement", r["precision"], r["recall"], gold)
    want = _results_of(gold)
    assert list(r["results"]) == list(want) and [float(v) for v in r["results"].values()] == list(want.values())


@pytest.mark.parametrize("case", ALL)
def test_cpu_path_reproduces_fixture(golden, case):
    from fiber_amd.modules import pack_detection_targets
    gold, k = golden(case), dv.case_inputs(case)
    ev = _evaluator(k)
    match, ignore, valid = ev.update(_tensors(k), pack_detection_targets(k["samples"], k["categories"]))
    _same_slots(case, "CPU path", match.numpy().view(np.uint64), ignore.numpy().view(np.uint64), valid.numpy(), gold, k)
    assert np.array_equal(ev.num_gt.numpy(), gold["num_gt"])
    precision, recall = ev.tables()
    _same_tables(case, "CPU path", precision.numpy(), recall.numpy(), gold)
    got, want = ev.summarize(), _results_of(gold)
    assert list(got) == list(want) and [float(v) for v in got.values()] == list(want.values())
    r = dv.restate(case)
    assert np.array_equal(match.numpy().view(np.uint64), r["match"]) and np.array_equal(valid.numpy(), r["valid"])


@pytest.mark.parametrize("case", ["apeval_small", "apeval_fixed", "apeval_edge"])
def test_two_updates_equal_one(golden, case):
    from fiber_amd.modules import pack_detection_targets
    gold, k = golden(case), dv.case_inputs(case)
    ev = _evaluator(k)
    B = len(k["samples"])
    G = max(len(s["annotations"]) for s in k["samples"])
    for sl in (slice(0, B // 2), slice(B // 2, B)):
        ev.update(_tensors(k, sl), pack_detection_targets(k["samples"][sl], k["categories"], num_boxes=G))
    precision, recall = ev.tables()
    _same_tables(case, "two updates", precision.numpy(), recall.numpy(), gold)
    assert [float(v) for v in ev.summarize().values()] == list(_results_of(gold).values())
    ev.reset()
    assert ev.image_ids == [] and int(ev.num_gt.sum()) == 0
    ev.update(_tensors(k), pack_detection_targets(k["samples"], k["categories"]))
    _same_tables(case, "after reset", *(t.numpy() for t in ev.tables()), gold)


def test_pack_detection_targets_layout():
    from fiber_amd.modules import pack_detection_targets
    k = dv.case_inputs("apeval_edge")
    t = pack_detection_targets(k["samples"], k["categories"], num_boxes=5)
    B = len(k["samples"])
    assert t.gt.shape == (B, 5, 4) and t.gt.dtype == torch.float64 and t.area.shape == (B, 5) and t.area.dtype == torch.float64
    assert t.category.dtype == torch.int32 and t.ignore.dtype == torch.uint8 and t.gt_count.dtype == torch.int32
    assert t.neg_mask.shape == (B, 1) and t.neg_mask.dtype == torch.int64 and t.nel_mask.shape == (B, 1)
    assert t.gt_count.tolist() == [0, 1, 2, 3, 3, 3] and t.image_ids == [10, 11, 12, 13, 14, 15]
    assert t.category_ids == [c["id"] for c in k["categories"]]
    assert t.gt[3, 1].tolist() == [104.0, 102.0, 50.0, 50.0] and t.category[3].tolist()[:3] == [1, 1, 4] and t.ignore[3].tolist()[:3] == [1, 0, 1]
    assert t.area[5, 1].item() == 9216.0 and t.neg_mask[:, 0].tolist() == [1, 0, 0, 0, 0, 0] and t.nel_mask[:, 0].tolist() == [0, 0, 8, 0, 0, 0]
    assert (t.gt[0] == 0).all() and (t.gt[1, 1:] == 0).all()
    wide = [dict(id=i + 1, frequency="f") for i in range(130)]              # three mask words; bit 63 is the sign bit of its int64
    s = [dict(image_id=1, annotations=[], neg_category_ids=[64, 130], not_exhaustive_category_ids=[1, 65])]
    t = pack_detection_targets(s, wide)
    assert t.neg_mask.shape == (1, 3) and t.neg_mask[0].tolist() == [-(1 << 63), 0, 2] and t.nel_mask[0].tolist() == [1, 1, 0]
    assert t.gt.shape == (1, 1, 4) and t.to("cpu").image_ids == [1]
    with pytest.raises(ValueError, match="num_boxes"):
        pack_detection_targets(k["samples"], k["categories"], num_boxes=2)
    with pytest.raises(ValueError, match="not in categories"):
        pack_detection_targets([dict(image_id=1, annotations=[dict(bbox=[0, 0, 5, 5], area=25.0, category_id=999)])], wide)
    with pytest.raises(ValueError, match="ascending"):
        pack_detection_targets(s, wide[::-1])
    with pytest.raises(ValueError, match="no extent"):
        pack_detection_targets([dict(image_id=1, annotations=[dict(bbox=[0, 0, 0, 5], area=25.0, category_id=1)])], wide)


def test_refusals():
    from fiber_amd.modules import BoxAPEvaluator, pack_detection_targets
    from fiber_amd.modules import detection_eval as de
    k = dv.case_inputs("apeval_small")
    assert de.MAX_GT >= 1024
    crowd = [dict(image_id=1, annotations=[dict(bbox=[i, 0, 5, 5], area=25.0, category_id=3) for i in range(de.MAX_GT + 1)])]
    with pytest.raises(ValueError, match="capacity"):
        pack_detection_targets(crowd, k["categories"])
    with pytest.raises(ValueError, match="64 bits"):                                       # T * A = 68 > 64
        BoxAPEvaluator(k["categories"], iou_thrs=np.linspace(0.1, 0.9, 17))
    BoxAPEvaluator(k["categories"], iou_thrs=np.linspace(0.1, 0.9, 16))
    with pytest.raises(ValueError, match="ascend"):
        BoxAPEvaluator(k["categories"], rec_thrs=[0.5, 0.1])
    with pytest.raises(ValueError):
        BoxAPEvaluator(k["categories"], fixed_ap_topk=0)
    ev = _evaluator(k)
    t = pack_detection_targets(k["samples"], k["categories"])
    ev.update(_tensors(k), t)
    ev.update(_tensors(k, slice(2, 3)), pack_detection_targets(k["samples"][2:3], k["categories"]))        # image 114 again
    with pytest.raises(ValueError, match="more than once"):
        ev.summarize()
    other = pack_detection_targets(k["samples"], k["categories"] + [dict(id=99, frequency="f")])
    with pytest.raises(ValueError, match="categories"):
        _evaluator(k).update(_tensors(k), other)
    with pytest.raises(ValueError, match="samples"):
        _evaluator(k).update(_tensors(k, slice(0, 2)), t)


def _sync_worker(rank, port, out_dir, case):
    import torch.distributed as dist
    from fiber_amd.modules import pack_detection_targets
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2)
    try:
        k = dv.case_inputs(case)
        B = len(k["samples"])
        sl = slice(0, B // 3) if rank == 0 else slice(B // 3, B)          # unequal shares: the gather pads to the largest
        ev = _evaluator(k)
        ev.update(_tensors(k, sl), pack_detection_targets(k["samples"][sl], k["categories"]))
        ev.synchronize()
        precision, recall = ev.tables()
        torch.save((precision, recall, ev.num_gt, ev.summarize(), ev.image_ids), os.path.join(out_dir, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case", ["apeval_small", "apeval_fixed"])
def test_synchronize_on_gloo_equals_single_process(golden, tmp_path, case):
    from fiber_amd.modules import pack_detection_targets
    gold, k = golden(case), dv.case_inputs(case)
    one = _evaluator(k)
    one.update(_tensors(k), pack_detection_targets(k["samples"], k["categories"]))
    one.synchronize()                                        # no process group: the identity
    want = one.summarize()
    mp_util.spawn_with_retry(_sync_worker, lambda port: (port, str(tmp_path), case), nprocs=2, deadline_s=120)
    for r in range(2):
        precision, recall, num_gt, res, ids = torch.load(os.path.join(str(tmp_path), f"r{r}.pt"), weights_only=False)
        _same_tables(case, f"rank {r}", precision.numpy(), recall.numpy(), gold)
        assert torch.equal(num_gt, one.num_gt) and res == want and sorted(ids) == sorted(one.image_ids)


def test_c_abi_exports_the_ap_entries():
    """The new symbols are exported from the built library, declared in the header and bound; at least 1024 ground truths per image."""
    from fiber_amd import lib, ops
    l = lib.load()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fiber_hip.h")).read()
    declared = set(re.findall(r"\b(?:int|long)\s+(fiber_\w+)\s*\(", hdr))
    for name in ("fiber_ap_match", "fiber_ap_accumulate", "fiber_ap_max_gt", "fiber_ap_chunk"):
        assert hasattr(l, name) and name in declared and name in lib.exported_symbols(), name
    from fiber_amd.modules import detection_eval as de
    assert ops.ap_max_gt() == de.MAX_GT >= 1024 and ops.ap_chunk() >= 1
