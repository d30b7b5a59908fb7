"""CPU tests of phrase-grounding evaluation: the scalar restatement of tests/ground_eval_cases.py and the CPU path of both evaluators
(fiber_amd/modules/grounding_eval.py) against tests/golden/geval_*.npz, which the reference's own Flickr30kEntitiesRecallEvaluator,
RefExpEvaluator, flickr_post_process, box_iou and generalized_box_iou produced (tools/gen_ground_eval_golden.py); the packing of
per-sample positive maps and of phrase targets with their refusals; duplicate and missing ids.  hit and counts exactly, best to 1 ulp
of its type (fp64 IoU, fp32 GIoU)."""
import types
import warnings

import numpy as np
import pytest
import torch

import ground_eval_cases as ge

FLICKR = [c for c, v in ge.CASES.items() if v["mode"] == 0]
_cache = {}


def _restated(case):
    if case not in _cache:
        det, samples, cats, topk, mode, merge = ge.case_inputs(case)
        _cache[case] = ge.restate(det.boxes, det.labels, det.count, samples, topk, ge.THRESH, mode, merge)
    return _cache[case]


def _gold_report(gold):
    rep = {}
    for k, c, v in zip(gold["report_k"].tolist(), gold["report_cat"].tolist(), gold["report_val"].tolist()):
        rep.setdefault(int(k), {})[c] = v
    return rep


def _check_best(case, got, gold, mode):
    live = gold["live"]
    dtype = np.float64 if mode == 0 else np.float32
    err = np.abs(got[live] - gold["best"][live])
    assert (err <= ge.ulp(gold["best"][live], dtype)).all(), f"{case}: best off by up to {err.max():.3e}"
    assert (got[~live] == 0).all(), f"{case}: a padding row carries a best"


def _tensors(det):
    ns = types.SimpleNamespace(labels=torch.from_numpy(det.labels), count=torch.from_numpy(det.count), scores=torch.from_numpy(det.scores))
    return torch.from_numpy(det.boxes), ns


def test_fixture_margins(golden):
    for case, c in ge.CASES.items():
        gold = golden(case)
        assert float(gold["margin_thresh"]) >= ge.MARGINS[c["mode"]] and float(gold["margin_scores"]) > 0
        for b, p in ge.EXACT[case]:
            assert (gold["best"][b, p] == ge.THRESH).all() and (gold["hit"][b, p] == 1).all()      # >= at the threshold exactly


@pytest.mark.parametrize("case", FLICKR)
def test_restatement_reproduces_flickr_fixture(golden, case):
    gold, r = golden(case), _restated(case)
    assert np.array_equal(r["hit"], gold["hit"]), f"{case}: hits differ"
    _check_best(case, r["best"], gold, 0)
    assert ge.report(r) == _gold_report(gold)                # the same integer counts divide to the same doubles
    if case == "geval_flickr_small":
        for (b, p), want in ge.FLICKR_EXPECT.items():
            assert tuple(r["hit"][b, p].tolist()) == want


def test_restatement_reproduces_refexp_fixture(golden):
    case = "geval_refexp"
    gold, r = golden(case), _restated(case)
    live = gold["live"]
    assert np.array_equal(r["hit"][live], gold["hit"][live])
    _check_best(case, np.where(live[..., None], r["best"], 0.0), gold, 1)
    assert (r["best"][3] == -1).all() and (r["hit"][3] == 0).all()       # no detection: a miss (the reference raises)
    assert float(r["best"][2].max()) < 0                                 # the negative GIoU
    det, samples, cats, topk, _, _ = ge.case_inputs(case)
    seen = gold["ref_images"].tolist()
    sub = ge.restate(det.boxes[seen], det.labels[seen], det.count[seen], [samples[b] for b in seen], topk, ge.THRESH, 1)
    assert ge.refexp_results(sub, cats, topk) == {n: v for n, v in zip(gold["results_name"].tolist(), gold["results_val"].tolist())}


@pytest.mark.parametrize("case", FLICKR)
def test_phrase_recall_evaluator_cpu(golden, case):
    from fiber_amd.modules.grounding_eval import PhraseRecallEvaluator
    gold = golden(case)
    det, samples, cats, topk, _, merge = ge.case_inputs(case)
    ev = PhraseRecallEvaluator(topk=topk, iou_thresh=ge.THRESH, merge_boxes=merge)
    boxes, ns = _tensors(det)
    hit, best = ev.update(boxes, ns, ev.targets_for(samples, cats))
    assert np.array_equal(hit.numpy(), gold["hit"])
    _check_best(case, best.numpy(), gold, 0)
    score = ev.summarize(expected_ids=[(s["image_id"], s["sentence_id"]) for s in samples])
    assert list(score) == gold["score_keys"].tolist()        # the reference's key names, in its order
    assert list(score.values()) == gold["score_vals"].tolist()
    assert ev.results == _gold_report(gold) == ev.report()
    r = _restated(case)
    pos, tot = ge.tables(r, cats, topk)
    assert np.array_equal(ev.positives.numpy(), pos) and np.array_equal(ev.totals.numpy(), tot)


def test_refexp_precision_evaluator_cpu(golden):
    from fiber_amd.modules.grounding_eval import RefExpPrecisionEvaluator
    case = "geval_refexp"
    gold = golden(case)
    det, samples, cats, topk, _, _ = ge.case_inputs(case)
    boxes, ns = _tensors(det)
    seen = gold["ref_images"].tolist()
    ev = RefExpPrecisionEvaluator(k=topk, thresh_iou=ge.THRESH)
    sub = types.SimpleNamespace(labels=ns.labels[seen], count=ns.count[seen])
    hit, best = ev.update(boxes[seen], sub, ev.targets_for([samples[b] for b in seen]))
    live = gold["live"]
    assert np.array_equal(hit.numpy(), gold["hit"][seen])
    assert (np.abs(best.numpy() - gold["best"][seen]) <= ge.ulp(gold["best"][seen], np.float32)).all()
    res = ev.summarize()
    assert list(res) == gold["results_name"].tolist() and [res[n] for n in res] == gold["results_val"].tolist()
    full = RefExpPrecisionEvaluator(k=topk, thresh_iou=ge.THRESH)      # all four images: the one without detections is a miss
    hit, best = full.update(boxes, ns, full.targets_for(samples))
    r = _restated(case)
    assert np.array_equal(hit.numpy(), r["hit"]) and np.array_equal(best.numpy(), r["best"])
    assert full.summarize() == ge.refexp_results(r, cats, topk)
    assert full.summarize()["refcoco"] == [0.0, 0.0, 0.5] and live.sum() == 3


def test_accumulation_over_updates_and_duplicates():
    from fiber_amd.modules.grounding_eval import PhraseRecallEvaluator
    det, samples, cats, topk, _, _ = ge.case_inputs("geval_flickr_small")
    boxes, ns = _tensors(det)
    one = PhraseRecallEvaluator(topk=topk)
    one.update(boxes, ns, one.targets_for(samples, cats))
    two = PhraseRecallEvaluator(topk=topk)
    for sl in (slice(0, 1), slice(1, 3)):
        part = types.SimpleNamespace(labels=ns.labels[sl], count=ns.count[sl])
        two.update(boxes[sl], part, two.targets_for(samples[sl], cats, num_phrases=5, num_boxes=3))
    assert torch.equal(one.positives, two.positives) and torch.equal(one.totals, two.totals)
    with pytest.warns(UserWarning, match="multiple predictions"):     # a repeated (image, sentence) is skipped
        part = types.SimpleNamespace(labels=ns.labels[:1], count=ns.count[:1])
        hit, _ = two.update(boxes[:1], part, two.targets_for(samples[:1], cats))
    assert int(hit.sum()) == 0 and torch.equal(one.totals, two.totals)
    assert one.summarize() == two.summarize()
    with pytest.raises(RuntimeError, match="Missing predictions"):
        one.summarize(expected_ids=[("1001", 0), ("9999", 3)])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fresh = PhraseRecallEvaluator(topk=topk)
        assert fresh.summarize() == {} and fresh.report() == {k: {} for k in topk}


def test_pack_phrase_targets_and_refusals():
    from fiber_amd.modules.grounding_eval import PhraseRecallEvaluator, RefExpPrecisionEvaluator, pack_phrase_targets
    samples = ge.flickr_samples()
    t = pack_phrase_targets(samples, ge.FLICKR_CATEGORIES)
    assert t.gt.shape == (3, 5, 3, 4) and t.gt.dtype == torch.float64 and t.gt_count.dtype == torch.int32 and t.cat_mask.dtype == torch.int64
    assert t.gt_count.tolist() == [[1, 1, 1, 1, 2], [1, 1, 1, 3, 0], [1, 2, 0, 0, 0]]
    assert t.categories[0] == "all" and t.image_ids == ["1001", "1002", "1003"]
    assert int(t.cat_mask[0, 4]) == 1 | 2 | 4 and int(t.cat_mask[1, 4]) == 0          # people + clothing; a padding row
    m = pack_phrase_targets(samples, ge.FLICKR_CATEGORIES, merge_boxes=True)
    assert m.gt.shape == (3, 5, 1, 4) and m.gt[0, 4, 0].tolist() == [300, 30, 620, 330] and int(m.gt_count.max()) == 1
    bad = [dict(image_id="x", sentence_id=0, phrases=[dict(boxes=[[5, 5, 5, 40]], phrase_type=["people"])])]
    with pytest.raises(ValueError, match="zero area"):
        pack_phrase_targets(bad, ge.FLICKR_CATEGORIES)
    with pytest.raises(ValueError, match="not in"):
        pack_phrase_targets([dict(image_id="x", sentence_id=0, phrases=[dict(boxes=[[0, 0, 5, 5]], phrase_type=["weather"])])], ge.FLICKR_CATEGORIES)
    with pytest.raises(ValueError, match="exceed"):
        pack_phrase_targets(samples, [f"c{i}" for i in range(64)])
    with pytest.raises(ValueError, match="num_phrases"):
        pack_phrase_targets(samples, ge.FLICKR_CATEGORIES, num_phrases=2)
    with pytest.raises(ValueError):
        PhraseRecallEvaluator(topk=tuple(range(1, 10)))      # K > 8
    with pytest.raises(ValueError):
        PhraseRecallEvaluator(topk=(1, 0))
    with pytest.raises(ValueError):
        RefExpPrecisionEvaluator(k=(1, -1))
    ev = RefExpPrecisionEvaluator()
    boxes, ns = _tensors(ge.flickr_detections())
    with pytest.raises(ValueError, match="ONE phrase"):
        ev.update(boxes, ns, t)


def test_pack_positive_maps_equals_per_sample_csr():
    from fiber_amd.modules.grounding_inference import PackedPositiveMaps, pack_positive_maps, positive_map_to_csr
    packed = pack_positive_maps(ge.MAPS, ge.MAPS_C)
    assert isinstance(packed, PackedPositiveMaps) and len(packed) == 3 and packed.num_classes == ge.MAPS_C
    assert packed.class_ptr.dtype == torch.int32 and packed.class_ptr.shape == (3, ge.MAPS_C + 1) and packed.tok_idx.dtype == torch.int32
    for b, m in enumerate(ge.MAPS):
        ptr, idx = positive_map_to_csr(m, ge.MAPS_C)
        row = packed.class_ptr[b]
        assert torch.equal(row - row[0], ptr)
        assert torch.equal(packed.tok_idx[int(row[0]):int(row[-1])], idx[:int(ptr[-1])])
        for c in range(ge.MAPS_C):                           # an unused class is an empty row
            assert (int(row[c + 1]) == int(row[c])) == (c + 1 not in m)
    assert int(packed.class_ptr[-1, -1]) == packed.tok_idx.numel()
    moved = packed.to("cpu")
    assert torch.equal(moved.class_ptr, packed.class_ptr) and torch.equal(moved.tok_idx, packed.tok_idx)
    v2 = pack_positive_maps([{1: 3, 2: [4, 5]}, {2: 9}], 4, v2=True)
    assert v2.class_ptr.tolist() == [[0, 1, 3, 3, 3], [3, 3, 4, 4, 4]] and v2.tok_idx.tolist() == [3, 4, 5, 9]
    with pytest.raises(TypeError):
        pack_positive_maps([{1: 3}], 4)                      # int entries are the v2 form
    with pytest.raises(ValueError):
        pack_positive_maps([{1: [3]}, {7: [4]}], 6)          # label outside 1..C
    with pytest.raises(ValueError):
        pack_positive_maps([{1: [256]}], 6)                  # token position outside 0..255
    with pytest.raises(ValueError):
        pack_positive_maps({1: [3]}, 6)                      # one dict is not a list of maps
    with pytest.raises(ValueError):
        pack_positive_maps([], 6)
    empty = pack_positive_maps([{}, {}], 3)
    assert empty.class_ptr.tolist() == [[0] * 4] * 2 and empty.tok_idx.numel() >= 1


def test_postprocessor_refuses_a_list_of_the_wrong_length():
    import detect_cases as dc
    from fiber_amd.modules.grounding_inference import BoxCoder, make_atss_postprocessor
    post = make_atss_postprocessor(dc.cfg_for("detect_small"), BoxCoder())
    x = dc.inputs("detect_small")
    sizes = torch.tensor(dc.CASES["detect_small"]["image_sizes"], dtype=torch.float32)
    with pytest.raises(ValueError, match="positive maps for a batch of 2"):
        post(x["bbox_reg"], x["centerness"], sizes, dc.anchors_for("detect_small"), x["logits"], ge.MAPS)


def test_evaluate_grounding_loop(golden):
    """The loop's wiring on CPU tensors: a stand-in model that returns the case's detections batch by batch and checks what it is called with."""
    from fiber_amd.modules.grounding_eval import PhraseRecallEvaluator, evaluate_grounding
    case = "geval_flickr_small"
    gold = golden(case)
    det, samples, cats, topk, _, _ = ge.case_inputs(case)
    boxes, ns = _tensors(det)
    ev = PhraseRecallEvaluator(topk=topk)
    calls = []

    class Images:
        def __init__(self, sl):
            self.sl = sl

        def boxes_to_original(self, detections):
            return detections.boxes * 1.0                    # (the case's boxes are in the original frame already)

    class Model:
        training = True

        def eval(self):
            self.training = False

        def __call__(self, images, tokenizer_input=None, positive_map=None):
            assert not self.training and not torch.is_grad_enabled()
            calls.append((tokenizer_input, len(positive_map)))
            return types.SimpleNamespace(boxes=boxes[images.sl], labels=ns.labels[images.sl], count=ns.count[images.sl])

    def batches():
        for sl in (slice(0, 2), slice(2, 3)):
            yield dict(images=Images(sl), tokenizer_input={"batch": sl.start}, positive_maps=[{1: [0]}] * (sl.stop - sl.start),
                       targets=ev.targets_for(samples[sl], cats))
    score = evaluate_grounding(Model(), batches(), ev, expected_ids=[(s["image_id"], s["sentence_id"]) for s in samples])
    assert calls == [({"batch": 0}, 2), ({"batch": 2}, 1)]
    assert list(score) == gold["score_keys"].tolist() and list(score.values()) == gold["score_vals"].tolist()
