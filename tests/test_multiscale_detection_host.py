"""Host tests of multi-scale test-time augmentation: the restatement of tests/multiscale_cases.py against fixtures the reference's own
box_aug.py / bounding_box.py produced (tools/gen_multiscale_golden.py), the numpy path of ops.det_aug_collect / ops.det_aug_merge against
the restatement, the tie orders the design states, mutations of the reference's rules that must not pass, and the refusals."""
import os
import types

import numpy as np
import pytest
import torch

import multiscale_cases as mc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALL_CASES = list(mc.VIEW_CASES) + list(mc.MERGE_CASES)


def golden(case, mode):
    return np.load(os.path.join(GOLDEN, mc.golden_name(case, mode) + ".npz"))


def case_inputs(case, mutate=None):
    """-> (cands per image, classes, top_n, junk)"""
    if case in mc.VIEW_CASES:
        c = mc.view_case(case)
        return mc.collect_ref(c, mutate), c["classes"], c["top_n"], False
    cands, classes, junk = mc.merge_case(case)
    return cands, classes, int(golden(case, "none")["top_n"]), junk


def same_as_fixture(result, g, mode):
    """the restatement's survivors against the reference's: counts, scores and labels exact; boxes exact ("none") or within vote_tol"""
    if [len(k) for k in result] != g["count"].tolist():
        return False
    for b, kept in enumerate(result):
        n = len(kept)
        if [np.float32(c["score"]) for c in kept] != g["scores"][b, :n].tolist() or [c["label"] for c in kept] != g["labels"][b, :n].tolist():
            return False
        if n == 0:
            continue
        mine = np.array([c["box"] for c in kept], np.float64)
        if mode == "none":
            if not np.array_equal(mine.astype(np.float32), g["boxes"][b, :n]):
                return False
        elif np.abs(mine - g["boxes"][b, :n]).max() > float(g["vote_tol"]):
            return False
    return True


@pytest.mark.parametrize("mode", mc.MODES)
@pytest.mark.parametrize("case", ALL_CASES)
def test_restatement_against_the_reference(case, mode):
    cands, classes, top_n, _ = case_inputs(case)
    g = golden(case, mode)
    result = mc.merge_ref(cands, classes, mc.TH, mode, top_n)
    assert same_as_fixture(result, g, mode)
    assert float(g["iou_margin"]) >= 1e-4 and float(g["score_gap"]) > 0
    if mode == "vote":
        assert float(g["vote_tol"]) > 0 and mc.voted_mask(result, top_n).any()


@pytest.mark.parametrize("case", list(mc.VIEW_CASES))
def test_unflip_range_resize_bit_exact(case):
    """every slot's box after the reference's transpose(0), remove_boxes and resize: the restatement and the numpy path of
    ops.det_aug_collect, both bit for bit; the cases hold ratio 1, equal ratios != 1 and unequal ratios"""
    from fiber_amd import ops
    c, g = mc.view_case(case), golden(case, "none")
    bx, sc, *_ = mc.cands_to_arrays(mc.collect_ref(c))
    assert np.array_equal(sc >= 0, g["t_live"]) and np.array_equal(bx.view(np.int32), g["t_boxes"].view(np.int32))
    out = mc.run_collect(ops, c, list(range(0, 16)), "cpu")                         # every label allowed: only the range filter drops
    assert np.array_equal(out[1].numpy() >= 0, g["t_live"]) and np.array_equal(out[0].numpy().view(np.int32), g["t_boxes"].view(np.int32))
    rows = [ops.det_aug_view_rows(c["originals"], v["sizes"], v["flip"], v["range"]) for v in c["views"]]
    assert {(r[1] == r[2], r[1] == 1.0) for view in rows for r in view} == {(True, True), (True, False), (False, False)}


@pytest.mark.parametrize("case", list(mc.VIEW_CASES))
def test_numpy_collect_against_the_restatement(case):
    from fiber_amd import ops
    c = mc.view_case(case)
    want = mc.cands_to_arrays(mc.filtered(mc.collect_ref(c), c["classes"]))
    got = mc.run_collect(ops, c, c["classes"], "cpu")
    for name, g, w in zip(("boxes", "scores", "labels", "source", "view"), got, want):
        assert np.array_equal(g.numpy(), w), name            # every slot written: no sentinel left


@pytest.mark.parametrize("mode", mc.MODES)
@pytest.mark.parametrize("case", ALL_CASES)
def test_numpy_merge_against_the_restatement(case, mode):
    from fiber_amd import ops
    cands, classes, top_n, junk = case_inputs(case)
    args = [torch.from_numpy(a) for a in mc.cands_to_arrays(cands, junk)]
    cls = torch.tensor(classes, dtype=torch.int32)
    tol = float(golden(case, "vote")["vote_tol"])
    survivors = max(len(k) for k in mc.merge_ref(cands, classes, mc.TH, mode, 1 << 30))
    for D in sorted({top_n, survivors, survivors + 3}):                          # the cut bites, fits exactly, leaves padding
        want = mc.merge_ref(cands, classes, mc.TH, mode, D)
        mc.assert_merge_equal(ops.det_aug_merge(*args, cls, mc.TH, mode, D), mc.result_arrays(want, D), mc.voted_mask(want, D), tol,
                           f"{case} {mode} D={D}")
    want = mc.merge_ref(cands, classes, 0.0, mode, top_n)                        # TH <= 0: nothing is suppressed
    mc.assert_merge_equal(ops.det_aug_merge(*args, cls, 0.0, mode, top_n), mc.result_arrays(want, top_n), mc.voted_mask(want, top_n), tol,
                       f"{case} {mode} TH=0")


def tie_case():
    """equal scores inside a class (ordered by view, then slot), across classes (the smaller label first) and at the cut"""
    far = lambda i: (100.0 * i, 0.0, 100.0 * i + 10, 10.0)                      # noqa: E731  (boxes that never touch)
    spec = [(far(0), 0.5, 3, 0), (far(1), 0.5, 2, 0), (far(2), 0.5, 2, 1), (far(3), 0.9, 2, 1), (far(4), 0.5, 3, 2), (far(5), 0.5, 2, 2),
            (far(6), 0.25, 1, 3)]
    return [[dict(box=b, score=s, label=l, source=10 + i, view=v, slot=i) for i, (b, s, l, v) in enumerate(spec)]]


@pytest.mark.parametrize("mode", mc.MODES)
def test_tie_orders_of_the_stated_deviations(mode):
    """score descending, then the smaller label, then the earlier slot (the slots of a view are contiguous and the views ascend, so this
    is: the earlier view, then the earlier slot); on a tie at the N-th score exactly N are kept, in that order"""
    from fiber_amd import ops
    cands = tie_case()
    args = [torch.from_numpy(a) for a in mc.cands_to_arrays(cands)]
    cls = torch.tensor([1, 2, 3], dtype=torch.int32)
    full = [3, 1, 2, 5, 0, 4, 6]                             # slots: 0.9; then 0.5 of label 2 by slot; then 0.5 of label 3; then 0.25
    for D in (7, 4, 3, 2):
        got = ops.det_aug_merge(*args, cls, mc.TH, mode, D)
        assert got[3][0].tolist() == [10 + s for s in full[:D]] and int(got[5][0]) == D
        want = mc.merge_ref(cands, [1, 2, 3], mc.TH, mode, D)
        assert [c["slot"] for c in want[0]] == full[:D]


MUTANT_KILLERS = {                                           # mutation: the (case, mode) whose fixture it must miss
    "nms_ge": ("views_select", "none"), "vote_gt": ("views_select", "vote"), "no_plus_one": ("views_norange", "none"),
    "range_nonstrict": ("views_select", "none"), "range_after_resize": ("views_select", "none"), "keep_other_labels": ("views_select", "none"),
}


@pytest.mark.parametrize("mutation", mc.MUTATIONS)
def test_mutations_are_rejected(mutation):
    case, mode = MUTANT_KILLERS[mutation]
    c = mc.view_case(case)
    g = golden(case, mode)
    assert same_as_fixture(mc.merge_ref(mc.collect_ref(c), c["classes"], mc.TH, mode, c["top_n"]), g, mode)
    mutant = mc.merge_ref(mc.collect_ref(c, mutation), c["classes"], mc.TH, mode, c["top_n"], mutation)
    assert not same_as_fixture(mutant, g, mode), mutation


def test_layout_case_holds_what_it_is_built_for():
    """the GPU merge case holds what tests/test_hip_multiscale_detection.py relies on"""
    cands, classes, junk = mc.merge_case("layout")
    assert len(cands) == 3 and junk and all(c is None for c in cands[2])
    sizes = [{l: sum(1 for c in slots if c is not None and c["label"] == l) for l in range(1, 9)} for slots in cands]
    assert sizes[0] == {1: 1, 2: 0, 3: 3, 4: 2, 5: 5, 6: 0, 7: mc.WG + 3, 8: 0}
    assert sizes[1] == {1: 4, 2: 2, 3: mc.WG + 5, 4: 3, 5: 0, 6: 0, 7: 0, 8: 2 * mc.WG}
    assert 4 not in classes and 3 in classes and 5 in classes
    kept = {m: mc.merge_ref(cands, classes, mc.TH, m, 1 << 30) for m in mc.MODES}
    chain = lambda m: sorted(c["score"] for c in kept[m][0] if c["label"] == 5 and c["box"][1] >= 200 and c["box"][1] < 300)   # noqa: E731
    assert [round(s, 2) for s in chain("none")] == [0.7, 0.9] and [round(s, 2) for s in chain("vote")] == [0.7, 0.9]     # C survives A's B
    pair = lambda m: [c for c in kept[m][0] if c["label"] == 5 and c["box"][0] == 300]                                     # noqa: E731
    assert len(pair("none")) == 2 and len(pair("vote")) == 1
    assert sum(1 for c in kept["vote"][1] if c["label"] == 3) == 1 and [c.get("members") for c in kept["vote"][1] if c["label"] == 3] == [mc.WG + 5]
    assert not any(c["label"] == 4 for m in mc.MODES for k in kept[m] for c in k)


def test_the_exact_threshold_pair_separates_the_two_rules():
    """[0, 0, 9, 9] and [0, 0, 9, 4]: IoU exactly 0.5 in fp32.  NMS (>) keeps both, the vote (>=) merges them."""
    from fiber_amd import ops
    a, b = mc.EXACT_PAIR
    assert np.float32(mc.iou(a, b)) == np.float32(0.5)
    cands = [[dict(box=a, score=0.75, label=1, source=1, view=0, slot=0), dict(box=b, score=0.25, label=1, source=2, view=1, slot=1)]]
    args = [torch.from_numpy(x) for x in mc.cands_to_arrays(cands)]
    cls = torch.tensor([1], dtype=torch.int32)
    kept = ops.det_aug_merge(*args, cls, 0.5, "none", 4)
    assert int(kept[5][0]) == 2 and kept[0][0, :2].tolist() == [list(a), list(b)]
    voted = ops.det_aug_merge(*args, cls, 0.5, "vote", 4)
    assert int(voted[5][0]) == 1 and voted[1][0, 0] == 0.75 and voted[3][0, 0] == 1 and voted[4][0, 0] == 0
    assert voted[0][0, 0].tolist() == [0.0, 0.0, 9.0, 0.75 * 9 + 0.25 * 4]      # exact in fp32
    assert voted[1][0, 1:].tolist() == [-1.0] * 3 and voted[4][0, 1:].tolist() == [-1] * 3


def test_refusals():
    from fiber_amd import ops
    args = [torch.from_numpy(a) for a in mc.cands_to_arrays(tie_case())]
    cls = torch.tensor([1, 2, 3], dtype=torch.int32)
    for soft in ("soft-nms", "soft-vote"):
        with pytest.raises(NotImplementedError, match=soft):
            ops.det_aug_merge(*args, cls, 0.5, soft, 4)
    with pytest.raises(ValueError, match="mode"):
        ops.det_aug_merge(*args, cls, 0.5, "nms", 4)
    with pytest.raises(ValueError, match="top_n"):
        ops.det_aug_merge(*args, cls, 0.5, "none", 0)
    with pytest.raises(ValueError, match="int32"):
        ops.det_aug_merge(args[0], args[1], args[2].long(), *args[3:], cls, 0.5, "none", 4)
    with pytest.raises(ValueError, match="classes"):
        ops.det_aug_merge(*args, cls.long(), 0.5, "none", 4)
    with pytest.raises(ValueError, match="capacity"):
        big = ops.DET_AUG_MAX_CANDIDATES + 1
        ops.det_aug_merge(torch.zeros(1, big, 4), torch.zeros(1, big), *(torch.zeros(1, big, dtype=torch.int32) for _ in range(3)), cls, 0.5,
                          "none", 4)
    assert ops.DET_AUG_MAX_CANDIDATES >= 24 * 16384
    # det_aug_collect: shapes, dtypes, the slot range
    cand = (torch.zeros(1, 4, 4), torch.zeros(1, 4), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.int32))
    rows = ops.det_aug_view_rows([(10, 20)], [(10, 20)], False, None)
    out = (torch.zeros(1, 6, 4), torch.zeros(1, 6), *(torch.zeros(1, 6, dtype=torch.int32) for _ in range(3)))
    ops.det_aug_collect(*cand, rows, cls, out, 2, 0)
    for bad in (dict(offset=3), dict(offset=-1), dict(view=-1), dict(rows=rows * 2), dict(out=out[:4]), dict(out=(out[0].double(),) + out[1:]),
                dict(cand=(cand[0], cand[1], cand[2].long(), cand[3])), dict(cand=(cand[0][:, :3],) + cand[1:])):
        a = {**dict(cand=cand, rows=rows, out=out, offset=2, view=0), **bad}
        with pytest.raises(ValueError):
            ops.det_aug_collect(*a["cand"], a["rows"], cls, a["out"], a["offset"], a["view"])


def test_a_config_with_multiscale_builds_and_refuses_what_is_out_of_scope():
    import fpn_cases as fc
    from fiber_amd.modules import GeneralizedVLRCNN
    from fiber_amd.modules.grounding_inference import ATSSPostProcessor, BoxCoder, make_atss_postprocessor
    cfg = fc.model_cfg(**{"TEST.USE_MULTISCALE": True})
    make_atss_postprocessor(cfg, BoxCoder())
    with pytest.raises(NotImplementedError, match="candidates"):                 # the constructor's own argument still refuses
        ATSSPostProcessor(0.05, 100, 0.6, 100, 0, 7, BoxCoder(), bbox_aug_enabled=True)
    model = GeneralizedVLRCNN(cfg).eval()
    test = dict(SCALES=(64,), RANGES=(), MAX_SIZE=100, FLIP=False, SPECIAL_NMS="none", TH=0.5, PRE_NMS_TOP_N=10, NUM_CLASSES=5, SELECT_CLASSES=())
    assert GeneralizedVLRCNN.multiscale_views(types.SimpleNamespace(SCALES=(40, 60), RANGES=((1, 2), (3, 4)), FLIP=True)) == \
        [(40, (1, 2), False), (40, (1, 2), True), (60, (3, 4), False), (60, (3, 4), True)]
    assert GeneralizedVLRCNN.multiscale_views(types.SimpleNamespace(SCALES=(40, 60), RANGES=((1, 2),), FLIP=False)) == \
        [(40, None, False), (60, None, False)]
    for bad, match in ((dict(PRE_NMS_TOP_N=0), "PRE_NMS_TOP_N"), (dict(PRE_NMS_TOP_N=-1), "PRE_NMS_TOP_N"), (dict(SPECIAL_NMS="soft-nms"), "soft-nms"),
                       (dict(SPECIAL_NMS="soft-vote"), "soft-vote")):
        with pytest.raises(NotImplementedError, match=match):
            model.detect_multiscale([], tokenizer_input={}, test_cfg=types.SimpleNamespace(**{**test, **bad}))
    model.train()
    with pytest.raises(RuntimeError, match="training mode"):
        model.detect_multiscale([], tokenizer_input={}, test_cfg=types.SimpleNamespace(**test))
