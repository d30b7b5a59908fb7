"""GPU tests of phrase-grounding evaluation: per-sample positive maps in the score kernel (fiber_det_scores_rows_f32) against per-sample
calls of the existing entry, bitwise, on NaN-filled outputs with guard words; ATSSPostProcessor with a list of maps against B = 1 calls of
the existing path; the recall kernel of csrc/geval.hip against the reference-run fixtures tests/golden/geval_*.npz and the scalar
restatement of tests/ground_eval_cases.py (hit and counts exactly, best to 1 ulp of its type, every element written, guards intact, two
runs bitwise equal, accumulation over updates); ABI refusals; VLDyHeadModule -> boxes_to_original -> evaluator end to end; one update
in a captured graph."""
import types

import numpy as np
import pytest
import torch

import detect_cases as dc
import ground_cases as gc
import ground_eval_cases as ge

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
NAN = float("nan")


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


_heads = {}


def _head_outputs():
    """detect_small's per-level head outputs with sample 0 repeated as sample 2 (B = 3), on the device, once"""
    if not _heads:
        x = dc.inputs("detect_small")
        _heads.update({k: [ge.three(t).to(DEV) for t in v] for k, v in x.items()})
        _heads["anchors"] = [a.to(DEV) for a in dc.anchors_for("detect_small")]
        sizes = dc.CASES["detect_small"]["image_sizes"]
        _heads["sizes"] = torch.tensor(sizes + sizes[:1], dtype=torch.float32, device=DEV)
    return _heads


@pytest.mark.parametrize("agg", ["MEAN", "MAX"])
def test_scores_rows_equal_per_sample_calls(lib, agg):
    from fiber_amd.modules.grounding_inference import pack_positive_maps, positive_map_to_csr
    h, C = _head_outputs(), ge.MAPS_C
    packed = pack_positive_maps(ge.MAPS, C).to(DEV)
    wide = torch.full((3, C + 4), -12345, dtype=torch.int32, device=DEV)       # the same rows at a stride above C + 1
    wide[:, :C + 1] = packed.class_ptr
    single = [tuple(t.to(DEV) for t in positive_map_to_csr(m, C)) for m in ge.MAPS]
    for l, (lg, ctr) in enumerate(zip(h["logits"], h["centerness"])):
        B, A, _ = lg.shape
        n = B * A * C
        want = torch.full((B, A, C), NAN, device=DEV)
        for b, (ptr, idx) in enumerate(single):
            lib.call("fiber_det_scores_f32", lib.ptr(lg[b:b + 1]), lib.ptr(ctr[b:b + 1]), lib.ptr(ptr), lib.ptr(idx), lib.ptr(want[b:b + 1]), 1, A,
                     dc.T, C, 0.05, int(agg == "MAX"))
        assert not bool(torch.isnan(want).any())
        for rows, stride in ((packed.class_ptr, C + 1), (wide, C + 4)):
            buf, out = _guarded(n, torch.float32, NAN)
            lib.call("fiber_det_scores_rows_f32", lib.ptr(lg), lib.ptr(ctr), lib.ptr(rows), lib.ptr(packed.tok_idx), lib.ptr(out), B, A, dc.T, C,
                     0.05, int(agg == "MAX"), stride)
            assert not bool(torch.isnan(out).any()) and _guard_intact(buf, n, NAN), f"level {l}: unwritten output or guard overwritten"
            assert torch.equal(out.view(B, A, C), want), f"level {l} stride {stride}: differs from the per-sample calls"
        assert bool((want[1, :, 2:] == -1).all()) and bool((want[0, :, 4] == -1).all()), "an unused class scores -1"
        assert bool((want[0] >= 0).any()) and not torch.equal(want[0], want[2]), "the repeated sample scores differently under its own map"
        ptr, idx = single[0]                                 # stride 0: one map for all = the old entry
        old = torch.full((B, A, C), NAN, device=DEV)
        lib.call("fiber_det_scores_f32", lib.ptr(lg), lib.ptr(ctr), lib.ptr(ptr), lib.ptr(idx), lib.ptr(old), B, A, dc.T, C, 0.05, int(agg == "MAX"))
        new = torch.full((B, A, C), NAN, device=DEV)
        lib.call("fiber_det_scores_rows_f32", lib.ptr(lg), lib.ptr(ctr), lib.ptr(ptr), lib.ptr(idx), lib.ptr(new), B, A, dc.T, C, 0.05,
                 int(agg == "MAX"), 0)
        assert torch.equal(old, new) and torch.equal(old[0], want[0])


def _post():
    from fiber_amd.modules.grounding_inference import BoxCoder, make_atss_postprocessor
    return make_atss_postprocessor(dc.cfg_for("detect_small"), BoxCoder())


def _run(post, h, maps, sl=slice(None)):
    return post([t[sl] for t in h["bbox_reg"]], [t[sl] for t in h["centerness"]], h["sizes"][sl], h["anchors"], [t[sl] for t in h["logits"]], maps)


def test_postprocessor_with_a_list_of_maps(lib):
    from fiber_amd import ops
    from fiber_amd.modules.grounding_inference import pack_positive_maps
    h, post = _head_outputs(), _post()
    det = _run(post, h, ge.MAPS)
    packed = pack_positive_maps(ge.MAPS, ge.MAPS_C).to(DEV)
    again = _run(post, h, packed)                            # already packed: no copy
    for b in range(3):
        one = _run(post, h, ge.MAPS[b], slice(b, b + 1))      # the existing path at B = 1
        for name in ("boxes", "scores", "labels", "source", "count"):
            got, want = getattr(det, name)[b:b + 1], getattr(one, name)
            assert torch.equal(got, want), f"image {b}: {name} differs from the B = 1 call"      # (equal NaN-free floats: bitwise)
            assert torch.equal(getattr(again, name)[b:b + 1], want)
        assert int(det.count[b]) > 0
    labs = det.labels[1, :int(det.count[1])]
    assert bool(((labs == 1) | (labs == 2)).all()), "sample 1's map has two classes"
    assert not torch.equal(det.source[0], det.source[2]), "the same image under two captions"
    with pytest.raises(ValueError):
        _run(post, h, ge.MAPS[:2])
    with pytest.raises(ValueError):
        _run(post, h, pack_positive_maps(ge.MAPS, ge.MAPS_C))                      # packed, but on the host
    with pytest.raises(ValueError):
        ops.det_scores(h["logits"][2], h["centerness"][2], packed.class_ptr[:2], packed.tok_idx, 0.05)


# ---- the recall kernel ------------------------------------------------------------------------------------------------------------------
_cases = {}


def _case(case):
    """device tensors, packed targets and the restatement, once per case"""
    if case not in _cases:
        from fiber_amd.modules.grounding_eval import pack_phrase_targets
        det, samples, cats, topk, mode, merge = ge.case_inputs(case)
        r = ge.restate(det.boxes, det.labels, det.count, samples, topk, ge.THRESH, mode, merge)
        t = pack_phrase_targets(samples, cats, merge_boxes=merge)
        _cases[case] = dict(det=types.SimpleNamespace(boxes=torch.from_numpy(det.boxes).to(DEV), labels=torch.from_numpy(det.labels).to(DEV),
                                                      count=torch.from_numpy(det.count).to(DEV)),
                            samples=samples, cats=cats, topk=topk, mode=mode, merge=merge, r=r, t=t.to(DEV), tables=ge.tables(r, cats, topk))
    return _cases[case]


def _launch(lib, k, hit, best, pos, tot):
    d, t = k["det"], k["t"]
    B, D = d.labels.shape
    P, G = t.gt.shape[1:3]
    topk = torch.tensor(k["topk"], dtype=torch.int32, device=DEV)
    lib.call("fiber_ground_recall", lib.ptr(d.boxes), lib.ptr(d.labels), lib.ptr(d.count), lib.ptr(t.gt), lib.ptr(t.gt_count), lib.ptr(t.cat_mask),
             lib.ptr(topk), lib.ptr(hit), lib.ptr(best), lib.ptr(pos), lib.ptr(tot), B, D, P, G, len(k["topk"]), len(t.categories), ge.THRESH,
             k["mode"])
    return B, P, len(k["topk"])


@pytest.mark.parametrize("case", list(ge.CASES))
def test_recall_kernel_against_fixture_and_restatement(lib, golden, case):
    gold, k = golden(case), _case(case)
    B, P = k["t"].gt_count.shape
    K = len(k["topk"])
    n = B * P * K
    runs = []
    for base in (0, 1000):                                   # the tables are added to, not written
        (hb, hit), (bb, best) = _guarded(n, torch.int32, -77), _guarded(n, torch.float64, NAN)
        (pb, pos), (tb, tot) = _guarded(K * 64, torch.int64, base), _guarded(K * 64, torch.int64, base)
        _launch(lib, k, hit, best, pos, tot)
        torch.cuda.synchronize()
        assert _guard_intact(hb, n, -77) and _guard_intact(bb, n, NAN) and _guard_intact(pb, K * 64, base) and _guard_intact(tb, K * 64, base)
        assert not bool(torch.isnan(best).any()) and not bool((hit == -77).any()), f"{case}: an element of hit / best was not written"
        runs.append((hit.view(B, P, K).cpu().numpy(), best.view(B, P, K).cpu().numpy(), pos.view(K, 64).cpu().numpy() - base,
                     tot.view(K, 64).cpu().numpy() - base))
    for a, b in zip(*runs):
        assert np.array_equal(a, b), f"{case}: two runs differ"
    hit, best, pos, tot = runs[0]
    r, live = k["r"], gold["live"]
    dtype = np.float64 if k["mode"] == 0 else np.float32
    assert np.array_equal(hit, r["hit"]) and np.array_equal(hit[live], gold["hit"][live]), f"{case}: hits"
    assert (np.abs(best - r["best"]) <= ge.ulp(r["best"], dtype)).all(), f"{case}: best against the restatement"
    assert (np.abs(best[live] - gold["best"][live]) <= ge.ulp(gold["best"][live], dtype)).all(), f"{case}: best against the reference"
    print(f"{case}: max |best - reference| {np.abs(best[live] - gold['best'][live]).max():.3e}")
    assert np.array_equal(pos, k["tables"][0]) and np.array_equal(tot, k["tables"][1]), f"{case}: counts"
    if k["mode"] == 0:
        pad = k["t"].gt_count.cpu().numpy() == 0
        assert pad.any() and (hit[pad] == 0).all() and (best[pad] == 0).all(), "padding rows are written as 0 / 0.0"
        for b, p in ge.EXACT[case]:
            assert (best[b, p] == ge.THRESH).all() and (hit[b, p] == 1).all()


@pytest.mark.parametrize("case", ["geval_flickr_small", "geval_refexp"])
def test_evaluators_accumulate_over_updates(lib, golden, case):
    from fiber_amd.modules.grounding_eval import PhraseRecallEvaluator, RefExpPrecisionEvaluator
    k = _case(case)
    make = (lambda: PhraseRecallEvaluator(topk=k["topk"])) if k["mode"] == 0 else (lambda: RefExpPrecisionEvaluator(k=k["topk"]))     # noqa: E731
    one, two = make(), make()
    hit, best = one.update(k["det"].boxes, k["det"], k["t"])
    assert np.array_equal(hit.cpu().numpy(), k["r"]["hit"])
    B = hit.shape[0]
    P, G = k["t"].gt.shape[1:3]
    for sl in (slice(0, 1), slice(1, B)):
        part = types.SimpleNamespace(labels=k["det"].labels[sl], count=k["det"].count[sl])
        two.update(k["det"].boxes[sl], part, two.targets_for(k["samples"][sl], *([k["cats"]] if k["mode"] == 0 else []), num_phrases=P, num_boxes=G).to(DEV))
    assert torch.equal(one.positives, two.positives) and torch.equal(one.totals, two.totals)
    assert np.array_equal(one.positives.cpu().numpy(), k["tables"][0]) and np.array_equal(one.totals.cpu().numpy(), k["tables"][1])
    gold = golden(case)
    if k["mode"] == 0:
        score = one.summarize(expected_ids=[(s["image_id"], s["sentence_id"]) for s in k["samples"]])
        assert list(score) == gold["score_keys"].tolist() and list(score.values()) == gold["score_vals"].tolist()
        with pytest.warns(UserWarning, match="multiple predictions"):
            hit, _ = two.update(k["det"].boxes, k["det"], k["t"])                  # every sample a repeat: nothing is counted
        assert int(hit.sum()) == 0 and torch.equal(one.totals, two.totals)
    else:
        assert one.summarize() == ge.refexp_results(k["r"], k["cats"], k["topk"]) == two.summarize()


def test_recall_abi_refusals(lib):
    k = _case("geval_flickr_small")
    d, t = k["det"], k["t"]
    B, D = d.labels.shape
    P, G = t.gt.shape[1:3]
    topk = torch.tensor([1, 5, 10, -1, 2, 3, 4, 6, 7], dtype=torch.int32, device=DEV)
    hit = torch.zeros(B * P * 9, dtype=torch.int32, device=DEV)
    best = torch.zeros(B * P * 9, dtype=torch.float64, device=DEV)
    pos, tot = torch.zeros((9, 64), dtype=torch.int64, device=DEV), torch.zeros((9, 64), dtype=torch.int64, device=DEV)

    def call(boxes=d.boxes, labels=d.labels, B=B, D=D, P=P, G=G, K=4, ncat=9, mode=0):
        lib.call("fiber_ground_recall", None if boxes is None else lib.ptr(boxes), None if labels is None else lib.ptr(labels), lib.ptr(d.count),
                 lib.ptr(t.gt), lib.ptr(t.gt_count), lib.ptr(t.cat_mask), lib.ptr(topk), lib.ptr(hit), lib.ptr(best), lib.ptr(pos), lib.ptr(tot),
                 B, D, P, G, K, ncat, ge.THRESH, mode)
    call()
    call(K=8)
    for bad in (dict(K=9), dict(K=-1), dict(ncat=65), dict(ncat=-1), dict(D=-1), dict(G=-1), dict(B=-1), dict(P=-1), dict(mode=2), dict(mode=-1),
                dict(mode=1), dict(labels=None), dict(boxes=None)):       # mode 1 takes P = 1 only; mode 0 reads labels
        with pytest.raises(lib.FiberHipError):
            call(**bad)
    with pytest.raises(lib.FiberHipError):                   # misaligned boxes
        lib.call("fiber_ground_recall", lib.ptr(d.boxes) + 4, lib.ptr(d.labels), lib.ptr(d.count), lib.ptr(t.gt), lib.ptr(t.gt_count),
                 lib.ptr(t.cat_mask), lib.ptr(topk), lib.ptr(hit), lib.ptr(best), lib.ptr(pos), lib.ptr(tot), B, D - 1, P, G, 4, 9, ge.THRESH, 0)
    before = tot.clone()
    lib.call("fiber_ground_recall", None, None, None, None, None, None, None, None, None, None, None, 0, D, P, G, 4, 9, ge.THRESH, 0)      # B == 0
    lib.call("fiber_ground_recall", None, None, None, None, None, None, None, None, None, None, None, B, D, 0, G, 4, 9, ge.THRESH, 0)      # P == 0
    call(labels=None, P=1, mode=1)                           # mode 1 does not read labels
    torch.cuda.synchronize()
    assert int((tot - before)[:4, 0].sum()) == 4 * B


def _module_cfg():
    cfg = gc.head_cfg(convs=gc.SMALL["convs"])
    d = dc.cfg_for("detect_small")
    for k, v in vars(d.MODEL.RPN).items():
        setattr(cfg.MODEL.RPN, k, v)
    cfg.MODEL.ATSS, cfg.MODEL.DYHEAD.SCORE_AGG, cfg.TEST = d.MODEL.ATSS, "MEAN", d.TEST
    cfg.TEST.MDETR_STYLE_AGGREGATE_CLASS_NUM = ge.MAPS_C     # the head has one class channel: the six labels need the v2 mapping's num_class
    return cfg


def test_module_to_evaluator_end_to_end(lib):
    """VLDyHeadModule on the ground_small weights with a map per sample, boxes_to_original, PhraseRecallEvaluator: equal to the restatement
    run on those same detections (copied to the host)."""
    from fiber_amd.data import DetImageList
    from fiber_amd.modules import PhraseRecallEvaluator, VLDyHeadModule
    m = VLDyHeadModule(_module_cfg())
    gc.set_head_weights(m.head)
    m = m.to(DEV).eval()
    xs, emb, _, _ = gc.small_inputs()
    xs, emb = [ge.three(x).to(DEV) for x in xs], ge.three(emb).to(DEV)
    sizes = [(160, 224), (150, 200), (160, 224)]             # (h, w) of the resized images
    images = DetImageList(None, sizes, [(480, 672, 0), (375, 500, 0), (240, 336, 0)])
    det = m(sizes, xs, {"embedded": emb}, ge.MAPS)
    boxes = images.boxes_to_original(det)
    hb, hl, hc = boxes.cpu().numpy(), det.labels.cpu().numpy(), det.count.cpu().numpy()
    assert (hc > 0).all()
    samples = []
    for b in range(3):                                       # ground truth made of this image's own detections, so that some phrases hit
        phrases = []
        for p in range(max(ge.MAPS[b])):
            mine = [i for i in range(int(hc[b])) if hl[b, i] == p + 1]
            src = hb[b, mine[min(2, len(mine) - 1)]] if mine else np.array([10.0, 20.0, 110.0, 90.0])
            box = [float(np.floor(src[0])), float(np.floor(src[1])), float(np.ceil(src[2])) + 1, float(np.ceil(src[3])) + 1]
            phrases.append(dict(boxes=[box, [400.0, 5.0, 470.0, 60.0]], phrase_type=[ge.FLICKR_CATEGORIES[p % 3]]))
        samples.append(dict(image_id=f"img{b}", sentence_id=b, phrases=phrases))
    ev = PhraseRecallEvaluator()
    hit, best = ev.update(boxes, det, ev.targets_for(samples, ge.FLICKR_CATEGORIES).to(DEV))
    r = ge.restate(hb, hl, hc, samples, ev.topk, 0.5, 0)
    P = hit.shape[1]
    assert np.array_equal(hit.cpu().numpy(), r["hit"][:, :P]) and int(r["hit"].sum()) > 0 and int((1 - r["hit"]).sum()) > 0
    assert (np.abs(best.cpu().numpy() - r["best"]) <= ge.ulp(r["best"], np.float64)).all()
    assert ev.report() == ge.report(r)
    score = ev.summarize()
    assert "Recall@1_all" in score and "Upper_bound_all" in score and score["Upper_bound_all"] >= score["Recall@1_all"]


def test_update_in_a_captured_graph(lib):
    """The post-processor with pre-packed maps and one evaluator update on a single stream, captured and replayed: the replay adds what the
    eager update adds."""
    from fiber_amd.modules.grounding_eval import PhraseRecallEvaluator, pack_phrase_targets
    from fiber_amd.modules.grounding_inference import pack_positive_maps
    h, post = _head_outputs(), _post()
    packed = pack_positive_maps(ge.MAPS, ge.MAPS_C).to(DEV)
    samples = [dict(image_id=f"g{b}", sentence_id=0,
                    phrases=[dict(boxes=[[20 + 30 * p, 10 + 20 * p, 120 + 30 * p, 90 + 20 * p]], phrase_type=["people"]) for p in range(max(ge.MAPS[b]))])
               for b in range(3)]
    targets = pack_phrase_targets(samples, ge.FLICKR_CATEGORIES).to(DEV)
    eager = PhraseRecallEvaluator()
    want_hit, want_best = eager.update(_run(post, h, packed).boxes, _run(post, h, packed), targets)
    ev = PhraseRecallEvaluator()

    def step():
        det = _run(post, h, packed)
        return ev.update(det.boxes, det, targets)            # (the resized frame taken as the original one: the ratio table is a host copy)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                               # warm-up on the capture stream: the tables and topk are allocated here
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    ev.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                # a single stream: no parallel branches
        hit, best = step()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(hit, want_hit) and torch.equal(best, want_best)
    assert torch.equal(ev.positives, eager.positives) and torch.equal(ev.totals, eager.totals) and int(ev.totals[0, 0]) == 14
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(ev.totals, 2 * eager.totals) and torch.equal(ev.positives, 2 * eager.positives)
