"""Grounding inference on the host: tests/detect_cases.py's plain-torch restatement against fixtures the REFERENCE's own ATSSPostProcessor
produced (tools/gen_detect_golden.py), the product's anchors and CSR conversion, and -- in the compare-host tradition -- mutations of the
restatement that must each be rejected."""
import numpy as np
import pytest
import torch

import detect_cases as dc

CASE_NAMES = list(dc.CASES)
_runs = {}


def _run(case, dtype=torch.float32, **mut):
    key = (case, dtype, tuple(sorted(mut.items())))
    if key not in _runs:
        _runs[key] = dc.run_case(case, dtype, **mut)
    return _runs[key]


def _fixture_sorted(gold, b):
    order = np.argsort(-gold[f"scores{b}"], kind="stable")
    return {k: gold[f"{k}{b}"][order] for k in ("boxes", "scores", "labels", "source")}


def _same_detections(r, gold, B):
    """exact labels and source indices in score order, and the count"""
    for b in range(B):
        g = _fixture_sorted(gold, b)
        n = int(r["count"][b])
        if n != len(g["scores"]) or not np.array_equal(r["source"][b, :n].numpy(), g["source"]) or \
                not np.array_equal(r["labels"][b, :n].numpy().astype(np.int64), g["labels"]):
            return False
    return True


@pytest.mark.parametrize("case", CASE_NAMES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_restatement_reproduces_the_reference(golden, case, dtype):
    gold, c = golden(case), dc.CASES[case]
    for k, v in dc.MARGINS.items():
        assert float(gold["margin_" + k]) >= v, f"{case}: fixture margin {k} {float(gold['margin_' + k]):.2e} below {v:.0e}"
    r = _run(case, dtype)
    r64 = _run(case, torch.float64)
    assert _same_detections(r, gold, c["B"]), f"{case}: labels / source indices differ from the reference's detections"
    for b in range(c["B"]):
        g = _fixture_sorted(gold, b)
        n = len(g["scores"])
        assert (r["scores"][b, n:] == -1).all() and (r["source"][b, n:] == -1).all() and (r["labels"][b, n:] == 0).all()
        # the reference ran in fp32: it and the fp32 restatement are each within the float bound of the fp64 evaluation
        ref64 = r64["scores"][b, :n]
        for name, got in (("reference", torch.from_numpy(g["scores"])), ("restatement", r["scores"][b, :n])):
            assert bool(((got.double() - ref64).abs() <= dc.score_bound(ref64)).all()), f"{case} image {b}: {name} scores outside the bound"
        bb = dc.box_bound(r64["mag"][b, :n])
        for name, got in (("reference", torch.from_numpy(g["boxes"])), ("restatement", r["boxes"][b, :n])):
            assert bool(((got.double() - r64["boxes"][b, :n]).abs() <= bb).all()), f"{case} image {b}: {name} boxes outside the bound"


def test_cases_reach_their_branches(golden):
    s, e = _run("detect_small", torch.float64), _run("detect_edge", torch.float64)
    gs = golden("detect_small")
    assert s["cand_scores"].shape[1] == 600 and e["cand_scores"].shape[1] == 60 and e["cand_scores"].shape[1] % 64
    assert all(bool((v[:, -1] >= 0).all()) for v in s["topk"][:2]), "the top-k cut bites on levels 0 and 1"
    assert bool((s["topk"][2][:, -1] < 0).all()), "level 2 ends in padding"
    assert (gs["survivors"] > 100).all() and (gs["candidates"] - gs["survivors"] > 100).all(), "NMS removes a sizeable share, > D survive"
    assert int(e["count"][0]) < dc.CASES["detect_edge"]["D"]
    W, H = dc.CASES["detect_edge"]["image_sizes"][0]
    src = e["source"][0, :int(e["count"][0])]
    a = (src >> dc.SRC_A_SHIFT) & 0x3FFFF
    out = e["boxes"][0, :int(e["count"][0])][a == 4]
    assert len(out) and bool((out[:, 0] == W - 1).all()) and bool((out[:, 2] == W - 1).all()), "anchor 4 decodes outside: clipped to the edge column"
    x = dc.inputs("detect_edge")
    assert float(x["bbox_reg"][0][0, 2, 1, 2]) / 5.0 > dc.CLIP and bool((a == 7).any())
    # per-image clipping differs
    assert float(s["boxes"][0, :, 2].max()) == 223.0 and float(s["boxes"][1, :, 2].max()) == 199.0


@pytest.mark.parametrize("case", CASE_NAMES)
def test_anchors_bit_for_bit(golden, case):
    gold = golden(case)
    for l, a in enumerate(dc.anchors_for(case)):
        assert a.dtype == torch.float32 and np.array_equal(a.numpy(), gold[f"anchors{l}"]), f"{case} level {l}"


def test_anchor_generator_cache_and_cell_anchors():
    from fiber_amd.modules.grounding_inference import AnchorGenerator, generate_anchors
    # the classic table of the 1-based original (quoted at anchor_generator.py:325-333) for stride 16, sizes 128 / 256 / 512, ratios
    # 0.5 / 1 / 2; the code works on the 0-based window (0, 0, 15, 15), hence every entry minus one
    want = [[-83, -39, 100, 56], [-175, -87, 192, 104], [-359, -183, 376, 200], [-55, -55, 72, 72], [-119, -119, 136, 136],
            [-247, -247, 264, 264], [-35, -79, 52, 96], [-79, -167, 96, 184], [-167, -343, 184, 360]]
    assert np.array_equal(generate_anchors(16, (128, 256, 512), (0.5, 1, 2)).numpy(), np.array(want, dtype=float) - 1)
    g = AnchorGenerator(((64,), (128,)), (1.0,), (8, 16))
    a, b = g.grid_anchors([(3, 5), (2, 2)]), g.grid_anchors([(3, 5), (2, 2)])
    assert a[0] is b[0] and a[0].shape == (15, 4) and g.num_anchors_per_location() == [1, 1]
    assert g.grid_anchors([(4, 5), (2, 2)])[0].shape == (20, 4)


def test_csr_of_both_map_forms():
    from fiber_amd.modules.grounding_inference import positive_map_to_csr
    ptr, idx = positive_map_to_csr(dc.CASES["detect_small"]["positive_map"], 6)
    assert ptr.tolist() == [0, 3, 5, 6, 11, 11, 14] and idx.tolist() == [3, 4, 5, 5, 6, 17, 30, 31, 32, 33, 200, 4, 31, 90]
    assert ptr.dtype == torch.int32 and idx.dtype == torch.int32
    ptr, idx = positive_map_to_csr({1: 3, 2: 10, 4: 200}, 4, v2=True)
    assert ptr.tolist() == [0, 1, 2, 2, 3] and idx.tolist() == [3, 10, 200]
    p2, i2 = positive_map_to_csr({1: [3], 2: [10], 4: [200]}, 4, v2=True)
    assert torch.equal(ptr, p2) and torch.equal(idx, i2)
    with pytest.raises(TypeError):
        positive_map_to_csr({1: 3}, 4)                       # int entries are the v2 form
    with pytest.raises(ValueError):
        positive_map_to_csr({5: [3]}, 4)
    with pytest.raises(ValueError):
        positive_map_to_csr({1: [256]}, 4)


def test_mask_words_layout():
    sup = torch.zeros((1, 70, 70), dtype=torch.bool)
    sup[0, 0, 1] = sup[0, 0, 63] = sup[0, 2, 64] = sup[0, 5, 69] = True
    w = dc.mask_words(sup)
    assert w.shape == (1, 70, 2) and int(w[0, 0, 0]) == (1 << 1) | -(1 << 63) and int(w[0, 2, 1]) == 1 and int(w[0, 5, 1]) == 1 << 5


# ---- mutations: each must be rejected ---------------------------------------------------------------------------------------------------
def _tie_case(**mut):
    """Four hand-made candidates of one label, descending scores, NMS 0.5.  Box 1 overlaps box 0 with IoU EXACTLY 0.5 under the +1
    convention (10 x 5 of 10 x 10): strict > keeps it.  Box 3 against box 2: 60 / 140 with the +1, 45 / 117 without (judged at NMS 0.4)."""
    boxes = torch.tensor([[[0, 0, 9, 9], [0, 0, 9, 4], [20, 20, 29, 29], [24, 20, 33, 29]]], dtype=torch.float64)
    scores = torch.tensor([[0.9, 0.8, 0.7, 0.6]], dtype=torch.float64)
    labels = torch.ones((1, 4), dtype=torch.int32)
    sup = dc.suppression(boxes, scores, labels, 0.5 if "plus_one" not in mut else 0.4, **mut)
    return dc.greedy_keep(sup, scores, 100)[0].tolist()


def test_mutation_ge_for_gt_is_rejected():
    assert _tie_case() == [True, True, True, True]           # IoU(0, 1) = 50 / 100 = 0.5, not > 0.5; IoU(2, 3) = 60 / 140
    assert _tie_case(ge=True) == [True, False, True, True]


def test_mutation_no_plus_one_is_rejected(golden):
    # IoU(2, 3) at NMS 0.4: with the +1, 6 x 10 / (200 - 60) = 0.4286 > 0.4; without, 5 x 9 / (162 - 45) = 0.3846
    assert _tie_case(plus_one=True) == [True, False, True, False]
    assert _tie_case(plus_one=False) == [True, False, True, True]
    assert not _same_detections(_run("detect_small", torch.float32, plus_one=False), golden("detect_small"), 2)


def test_mutation_candidate_test_after_centerness_is_rejected(golden):
    # detect_edge keeps every candidate (fewer than D survive): one whose agg passes the threshold and whose product with the centerness
    # does not is in the reference's detections and not in the mutant's
    assert not _same_detections(_run("detect_edge", torch.float32, after_ctr=True), golden("detect_edge"), 1)


def test_mutation_label_blind_nms_is_rejected(golden):
    assert not _same_detections(_run("detect_small", torch.float32, label_blind=True), golden("detect_small"), 2)


def test_unsupported_configurations_raise():
    from fiber_amd.modules.grounding_inference import ATSSPostProcessor, BoxCoder, make_atss_postprocessor
    kw = dict(pre_nms_thresh=0.05, pre_nms_top_n=100, nms_thresh=0.6, fpn_post_nms_top_n=100, min_size=0, num_classes=7, box_coder=BoxCoder())
    for bad in (dict(score_agg="POWER"), dict(score_agg="ONEHOT"), dict(bbox_aug_enabled=True), dict(nms_thresh=0.0)):
        with pytest.raises(NotImplementedError):
            ATSSPostProcessor(**{**kw, **bad})
    post = make_atss_postprocessor(dc.cfg_for("detect_small"), BoxCoder())
    assert (post.pre_nms_thresh, post.pre_nms_top_n, post.nms_thresh, post.fpn_post_nms_top_n, post.score_agg) == (0.05, 200, 0.6, 100, "MEAN")
    x = dc.inputs("detect_edge")
    with pytest.raises(NotImplementedError):
        post(x["bbox_reg"], x["centerness"], None, None, x["logits"], {1: [3]}, token_logits=x["logits"])
    with pytest.raises(NotImplementedError):
        post(x["bbox_reg"], x["centerness"], None, None, None, {1: [3]}, box_cls=x["logits"])
    with pytest.raises(NotImplementedError):
        post([torch.zeros(1, 8, 3, 5)], x["centerness"], None, None, x["logits"], {1: [3]})


def test_box_coder_decode_matches_the_restatement():
    from fiber_amd.modules.grounding_inference import BoxCoder
    x, anc = dc.inputs("detect_edge"), dc.anchors_for("detect_edge")[0]
    reg = x["bbox_reg"][0][0].reshape(4, -1).t().contiguous().double()
    got = BoxCoder().decode(reg, anc.double())
    flat = torch.arange(15)[None] * 4
    box = dc.decode(torch.ones(1, 15, dtype=torch.float64), flat, x["bbox_reg"][0], anc, torch.tensor([[1e6, 1e6]]), 4, 0)[0][0]
    assert torch.allclose(got.clamp_min(0), box, rtol=0, atol=1e-9)


def test_csr_cache_is_bounded():
    from fiber_amd.modules.grounding_inference import BoxCoder, make_atss_postprocessor
    post = make_atss_postprocessor(dc.cfg_for("detect_small"), BoxCoder())
    first = post.csr({1: [0]}, 6, "cpu")
    assert post.csr({1: [0]}, 6, "cpu")[0] is first[0]
    for t in range(1, post.CSR_CACHE + 4):
        post.csr({1: [t]}, 6, "cpu")
        post.csr({1: [0]}, 6, "cpu")                         # kept alive by use
    assert len(post._csr) == post.CSR_CACHE and post.csr({1: [0]}, 6, "cpu")[0] is first[0]
    assert post.csr({1: [1]}, 6, "cpu")[1].tolist() == [1]   # evicted long ago, rebuilt
