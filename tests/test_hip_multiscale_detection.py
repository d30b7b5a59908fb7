"""GPU tests of multi-scale test-time augmentation: fiber_det_aug_collect and fiber_det_aug_merge against the independent restatement of
tests/multiscale_cases.py (exact under plain NMS, within the fixtures' vote_tol for voted boxes, two runs bitwise equal), and
GeneralizedVLRCNN.detect_multiscale end to end on the tiny model: against the restatement applied to the model's own per-view candidates,
and, with one view that changes nothing, against the plain forward.  Where two executions of the head are compared exactly the second is
handed the first one's head outputs: the head's one-channel 1 x 1 convolutions do not give the same last bit twice
(profiles/chunked_detection.md)."""
import os
import types

import numpy as np
import pytest
import torch

import chunk_cases as cc
import det_input_cases as di
import multiscale_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from fiber_amd import lib as L
    L.load()
    return L


@pytest.fixture(scope="module")
def vote_tol():
    return float(np.load(os.path.join(GOLDEN, mc.golden_name("mid", "vote") + ".npz"))["vote_tol"])


_REFERENCE = {}


def reference(case, mode, D):
    """the restatement's result, computed once per (case, mode) and cut per D"""
    if (case, mode) not in _REFERENCE:
        cands, classes, _ = mc.merge_case(case)
        _REFERENCE[case, mode] = mc.merge_ref(cands, classes, mc.TH, mode, 1 << 30)
    return [k[:D] for k in _REFERENCE[case, mode]]


# ---- the merge --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", mc.MODES)
@pytest.mark.parametrize("case", list(mc.MERGE_CASES))
def test_merge_kernel_against_the_restatement(lib, vote_tol, case, mode):
    """layout: B = 3, segments of 0, 1, 2, 3, WG + 3 and 2 WG slots, a cluster of WG + 5, the chain, the exact-threshold pair, a label
    outside the table between allowed ones, an image without a live candidate, junk in the dead slots; mid: T = 24 x 600, 40 classes.
    top_n below, equal to and above the largest survivor count."""
    from fiber_amd import ops
    cands, classes, junk = mc.merge_case(case)
    args = [torch.from_numpy(a).to(DEV) for a in mc.cands_to_arrays(cands, junk)]
    cls = torch.tensor(classes, dtype=torch.int32, device=DEV)
    most = max(len(k) for k in reference(case, mode, 1 << 30))
    assert most > 3
    for D in (most // 2, most, most + 5):
        want = reference(case, mode, D)
        got = ops.det_aug_merge(*args, cls, mc.TH, mode, D)
        mc.assert_merge_equal(got, mc.result_arrays(want, D), mc.voted_mask(want, D), vote_tol, f"{case} {mode} D={D}")
        again = ops.det_aug_merge(*args, cls, mc.TH, mode, D)
        assert all(torch.equal(a, b) for a, b in zip(got, again)), f"{case} {mode} D={D}: two runs differ"
    if mode == "vote":
        assert mc.voted_mask(reference(case, mode, most), most).any()


@pytest.mark.parametrize("mode", mc.MODES)
@pytest.mark.parametrize("case", list(mc.VIEW_CASES))
def test_collect_and_merge_on_the_view_cases(lib, vote_tol, case, mode):
    from fiber_amd import ops
    c = mc.view_case(case)
    want = mc.cands_to_arrays(mc.filtered(mc.collect_ref(c), c["classes"]))
    got = mc.run_collect(ops, c, c["classes"], DEV)          # buffers pre-filled with a sentinel: every slot is written
    for name, g, w in zip(("boxes", "scores", "labels", "source", "view"), got, want):
        assert np.array_equal(g.cpu().numpy().view(np.int32), w.view(np.int32)), (case, name)
    cls = torch.tensor(c["classes"], dtype=torch.int32, device=DEV)
    for thresh in (mc.TH, 0.0):                              # TH <= 0: no launch, nothing suppressed
        ref = mc.merge_ref(mc.collect_ref(c), c["classes"], thresh, mode, c["top_n"])
        mc.assert_merge_equal(ops.det_aug_merge(*got, cls, thresh, mode, c["top_n"]), mc.result_arrays(ref, c["top_n"]),
                              mc.voted_mask(ref, c["top_n"]), vote_tol, f"{case} {mode} TH={thresh}")


def test_abi_refusals(lib):
    from fiber_amd import ops
    cap = int(lib.plain("fiber_det_aug_max_candidates"))
    assert cap == ops.DET_AUG_MAX_CANDIDATES and cap >= 24 * int(lib.plain("fiber_det_max_candidates"))
    B, Nv, T, C = 2, 8, 24, 3
    fi, fo = (torch.zeros(B * T * 4 + 8, dtype=torch.float32, device=DEV) for _ in range(2))
    ii, table, ic = (torch.zeros(B * T + 8, dtype=torch.int32, device=DEV) for _ in range(3))
    o1, o2, o3, o4 = (torch.zeros(B * T + 8, dtype=torch.int32, device=DEV) for _ in range(4))
    p = lib.ptr
    good = [p(fi), p(fi), p(ii), p(ii), p(table), p(ic), p(fo), p(o1), p(o2), p(o3), p(o4), B, Nv, T, 8, 1, C]
    lib.call("fiber_det_aug_collect", *good)
    bad = [{11: -1}, {11: 65536}, {13: cap + 1}, {14: T - Nv + 1}, {14: -1}, {15: -1}, {16: -1}, {0: p(fi) + 4}, {6: p(fo) + 8}, {1: p(fi) + 2},
           {4: p(table) + 2}] + [{n: None} for n in range(11)]
    for change in bad:
        args = list(good)
        for at, v in change.items():
            args[at] = v
        with pytest.raises(lib.FiberHipError):
            lib.call("fiber_det_aug_collect", *args)
    lib.call("fiber_det_aug_collect", *([None] * 11), 0, Nv, T, 0, 0, C)         # B == 0
    ii.fill_(1 << 30)                                        # every slot dead: no class has a segment
    good = [p(fi), p(fi), p(ii), p(ic), p(o1), p(fo), B, T, C, 0.5, 0]
    lib.call("fiber_det_aug_merge", *good)
    bad = [{6: -1}, {6: 65536}, {7: cap + 1}, {8: -1}, {9: 0.0}, {9: -1.0}, {9: float("nan")}, {10: 2}, {10: -1}, {0: p(fi) + 4}, {5: p(fo) + 8},
           {4: p(o1) + 2}] + [{n: None} for n in range(6)]
    for change in bad:
        args = list(good)
        for at, v in change.items():
            args[at] = v
        with pytest.raises(lib.FiberHipError):
            lib.call("fiber_det_aug_merge", *args)
    lib.call("fiber_det_aug_merge", *([None] * 6), 0, T, C, 0.5, 0)              # B == 0
    lib.call("fiber_det_aug_merge", *([None] * 6), B, T, 0, 0.5, 1)              # C == 0
    torch.cuda.synchronize()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------
SHAPES = ((64, 96), (80, 64))                                # (H, W): both keep their size at scale 64
POSITIVE_MAP = {1: [1, 2], 2: [4], 3: 7, 4: [5, 6]}          # TEST.MDETR_STYLE_AGGREGATE_CLASS_NUM = 4 classes


@pytest.fixture(scope="module")
def detector(lib):
    model = cc.make_detector((2, 2, 2, 2), DEV)
    di.input_cfg(model.cfg, divisible=32)
    return model


@pytest.fixture(scope="module")
def inputs():
    from fiber_amd import data
    g = np.random.default_rng(9)
    images = [torch.from_numpy(g.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(DEV) for H, W in SHAPES]
    ids = [torch.tensor([0] + list(range(100, 107)) + [2]), torch.tensor([0] + list(range(200, 212)) + [2])]
    tok = {k: v.to(DEV) for k, v in data.pad_input_ids(ids, 256, True).items()}
    return images, tok


def make_test_cfg(detector, **over):
    a = detector.cfg.MODEL.ATSS
    base = dict(SCALES=(64,), RANGES=(), MAX_SIZE=133, FLIP=False, SPECIAL_NMS="none", TH=a.NMS_TH, PRE_NMS_TOP_N=a.DETECTIONS_PER_IMG,
                NUM_CLASSES=5, SELECT_CLASSES=())
    return types.SimpleNamespace(**{**base, **over})


class Recorder:
    """records what detect_multiscale hands to ops.det_aug_collect: the model's own per-view candidates"""

    def __init__(self, monkeypatch):
        from fiber_amd import ops
        self.views = []
        real = ops.det_aug_collect

        def collect(boxes, scores, labels, source, rows, classes, out, offset, view):
            self.views.append((boxes, scores, labels, source, rows, offset, view))
            return real(boxes, scores, labels, source, rows, classes, out, offset, view)
        monkeypatch.setattr(ops, "det_aug_collect", collect)


@pytest.mark.parametrize("mode", mc.MODES)
def test_detect_multiscale_against_the_restatement(detector, inputs, vote_tol, monkeypatch, mode):
    """(a) two images of different sizes, two scales, flip on, a range per scale: the device result is the restatement applied to the
    candidates the model produced in each view"""
    from fiber_amd import data
    from fiber_amd.modules import Detections
    images, tok = inputs
    t = make_test_cfg(detector, SCALES=(48, 64), RANGES=((0, 1000), (6, 48)), FLIP=True, SPECIAL_NMS=mode, TH=0.5, PRE_NMS_TOP_N=30, NUM_CLASSES=4)
    rec = Recorder(monkeypatch)
    det = detector.detect_multiscale(images, tokenizer_input=tok, positive_map=POSITIVE_MAP, test_cfg=t)
    assert isinstance(det, Detections) and det.chunk is None and det.scores.shape == (2, 30) and len(rec.views) == 4
    views, off = [], 0
    for v, (boxes, scores, labels, source, rows, offset, view) in enumerate(rec.views):
        scale, keep, flip = ((48, (0, 1000)), (64, (6, 48)))[v // 2] + (bool(v % 2),)
        sizes = [data.det_resize_size(W, H, scale, 133) for H, W in SHAPES]
        assert (offset, view) == (off, v) and [r[0] for r in rows] == [float(s[1]) for s in sizes] and [bool(r[4]) for r in rows] == [flip] * 2
        views.append(dict(sizes=sizes, flip=flip, range=keep, boxes=boxes.cpu().tolist(), scores=scores.cpu().tolist(),
                          labels=labels.cpu().tolist(), source=source.cpu().tolist()))
        off += scores.shape[1]
    cands = mc.collect_ref(dict(originals=list(SHAPES), views=views))
    want = mc.merge_ref(cands, [1, 2, 3], 0.5, mode, 30)                         # label 4 is produced and dropped
    got = (det.boxes, det.scores, det.labels, det.source, det.view, det.count)
    mc.assert_merge_equal(got, mc.result_arrays(want, 30), mc.voted_mask(want, 30), vote_tol, f"end to end {mode}")
    live = [c for slots in cands for c in slots if c is not None]
    assert {c["view"] for k in want for c in k} >= {0, 1, 2, 3} and any(c["label"] == 4 for c in live) and int(det.count.min()) > 3
    assert any(s is None for slots in cands for s in slots)                    # (padding, or dropped by the range filter)
    if mode == "vote":
        assert mc.voted_mask(want, 30).any()


def test_one_unchanged_view_is_the_plain_forward(detector, inputs, monkeypatch):
    """(b) one scale that leaves both images as they are, no flip, TH = NMS_TH, PRE_NMS_TOP_N = DETECTIONS_PER_IMG, every class: the same
    set of (box, score, label), bit for bit, as model(...) followed by boxes_to_original"""
    from fiber_amd import data
    images, tok = inputs
    t = make_test_cfg(detector)
    assert [data.det_resize_size(W, H, 64, 133) for H, W in SHAPES] == list(SHAPES)
    rec, head = Recorder(monkeypatch), []
    handle = detector.rpn.head.register_forward_hook(lambda m, a, out: head.append((a[0], out)))
    try:
        det = detector.detect_multiscale(images, tokenizer_input=tok, positive_map=POSITIVE_MAP, test_cfg=t)
    finally:
        handle.remove()
    assert len(head) == 1 and bool((det.view[det.scores >= 0] == 0).all())

    def replay(m, a, out):
        assert all(torch.equal(x, y) for x, y in zip(a[0], head[0][0])), "the plain forward's features differ from the view's"
        return head[0][1]
    handle = detector.rpn.head.register_forward_hook(replay)
    try:
        batch = data.DeviceDetectionTransform.for_views(detector.cfg).apply(images, list(SHAPES), [False, False])
        with torch.no_grad():
            plain = detector(batch, tokenizer_input=tok, positive_map=POSITIVE_MAP)
    finally:
        handle.remove()
    back = batch.boxes_to_original(plain)
    tied = 0
    for b in range(2):
        s = rec.views[0][1][b].cpu().numpy()
        s = s[s >= 0]
        if len(set(s.tolist())) != len(s):
            tied += 1
            continue
        n, m = int(plain.count[b]), int(det.count[b])
        assert n == m and n > 3
        a = sorted(zip(back[b, :n].cpu().numpy().view(np.int32).tolist(), plain.scores[b, :n].tolist(), plain.labels[b, :n].tolist()), key=str)
        c = sorted(zip(det.boxes[b, :m].cpu().numpy().view(np.int32).tolist(), det.scores[b, :m].tolist(), det.labels[b, :m].tolist()), key=str)
        assert a == c, f"image {b}"
    assert tied <= 0


def test_evaluate_detection_multiscale(detector, inputs, monkeypatch):
    from fiber_amd.modules import BoxAPEvaluator, evaluate_detection_multiscale, pack_detection_targets
    images, tok = inputs
    monkeypatch.setattr(detector.cfg, "TEST", make_test_cfg(detector, SCALES=(48, 64), FLIP=True, SPECIAL_NMS="vote", TH=0.5, USE_MULTISCALE=True,
                                                       MDETR_STYLE_AGGREGATE_CLASS_NUM=4))
    cats = [dict(id=i, frequency="rcf"[i % 3]) for i in (3, 5, 8, 13)]
    det = detector.detect_multiscale(images, tokenizer_input=tok, positive_map=POSITIVE_MAP)
    hb, hl, hc = det.boxes.cpu().numpy(), det.labels.cpu().numpy(), det.count.cpu().numpy()
    samples = []
    for b in range(2):                                       # every third detection, grown by a pixel, is a ground truth of its category
        anns = []
        for i in range(0, int(hc[b]), 3):
            x1, y1, x2, y2 = [float(v) for v in hb[b, i]]
            w, h = float(np.ceil(x2 - x1)) + 1, float(np.ceil(y2 - y1)) + 1
            anns.append(dict(bbox=[float(np.floor(x1)), float(np.floor(y1)), w, h], area=w * h, category_id=cats[int(hl[b, i]) - 1]["id"]))
        samples.append(dict(image_id=b, annotations=anns, neg_category_ids=[], not_exhaustive_category_ids=[]))
    targets = pack_detection_targets(samples, cats).to(DEV)
    ev = BoxAPEvaluator(cats, max_dets=20)
    batches = [dict(images=images, tokenizer_input=tok, positive_maps=POSITIVE_MAP, targets=targets)]
    first = evaluate_detection_multiscale(detector, batches, ev)                 # (also: every lazily built table now exists)
    assert first["AP"] > 0 and int(ev.num_gt.sum()) > 0
    ev.reset()
    mode = torch.cuda.get_sync_debug_mode()
    summarize = ev.summarize

    def leave_then_summarize():
        torch.cuda.set_sync_debug_mode(mode)
        return summarize()
    ev.summarize = leave_then_summarize
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                  # nothing synchronises before summarize
    try:
        res = evaluate_detection_multiscale(detector, batches, ev)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert res["AP"] > 0 and int(ev.num_gt.sum()) > 0
