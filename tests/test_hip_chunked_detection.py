"""GPU tests of chunked open-vocabulary detection: the merge kernel (fiber_det_merge) against ops.det_merge's host path on sentinel-filled
outputs; the split backbone forward against the forward it was cut out of, bit for bit; the pair batch against the replicated batch within
the forward's own measured sensitivity to batch size; GeneralizedVLRCNN.detect_chunked against the existing head called pair by pair and
merged on the host; evaluate_detection_chunked against an evaluator fed those host-merged detections, at LVIS width too.  Where two
executions of the head are compared exactly, the second is handed the first one's head outputs (HeadTape says why)."""
import math

import numpy as np
import pytest
import torch

import chunk_cases as cc
import fpn_cases as fc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from fiber_amd import lib as L
    L.load()
    return L


@pytest.fixture(scope="module")
def shallow(lib):
    return cc.make_detector((2, 2, 2, 2), DEV)


@pytest.fixture(scope="module")
def deep(lib):
    return cc.make_detector((2, 2, 18, 2), DEV)              # fused blocks inside stage 2


@pytest.fixture(scope="module")
def prompts():
    return cc.pair_prompts().to(DEV)


# ---- the merge kernel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.MERGE_CASES) + list(cc.MERGE_CASES_GPU))
def test_merge_kernel_against_host_path(lib, name):
    from fiber_amd import ops
    x = cc.merge_inputs(name)
    want = ops.det_merge(*cc.merge_args(x))
    if name in cc.MERGE_CASES:                               # (held by the host tests for every case; repeated where it is cheap)
        assert all(torch.equal(a, b) for a, b in zip(want, cc.merge_ref(*cc.merge_args(x))))
    dev = [t.to(DEV) for t in cc.merge_args(x)[:6]]
    for sentinel in (-77, 77):                               # every element is written, whatever lay there
        out = tuple(torch.full(t.shape, sentinel, dtype=t.dtype, device=DEV) for t in want)
        got = ops.det_merge(*dev, x["max_dets"], out=out)
        for field, g, w in zip(cc.MERGE_FIELDS, got, want):
            assert g.dtype == w.dtype and torch.equal(g.cpu(), w), f"{name}: {field} (sentinel {sentinel})"
    fresh = ops.det_merge(*dev, x["max_dets"])               # torch.empty outputs
    assert all(torch.equal(g.cpu(), w) for g, w in zip(fresh, want)), name


def test_merge_abi_refusals(lib):
    from fiber_amd import ops
    cap = int(lib.plain("fiber_det_merge_max_candidates"))
    assert cap == ops.DET_MERGE_MAX_CANDIDATES
    B, K, D, Cc = 1, 2, 8, 3
    f = torch.zeros(B * K * D * 4 + 8, dtype=torch.float32, device=DEV)
    i = torch.zeros(B * K * D + 8, dtype=torch.int32, device=DEV)
    p = lib.ptr
    good = [p(f), p(f), p(i), p(i), p(i), p(i), p(f), p(f), p(i), p(i), p(i), p(i), B, K, D, Cc, K * D]
    lib.call("fiber_det_merge", *good)
    bad = [{12: -1}, {13: 65, 14: 1, 16: 65}, {13: 2, 14: cap // 2 + 1, 16: 1}, {16: K * D + 1}, {16: 0}, {15: -1},
           {0: p(f) + 4}, {6: p(f) + 8}, {1: p(f) + 2}, {11: p(i) + 1}] + [{n: None} for n in range(12)]
    for change in bad:
        args = list(good)
        for at, v in change.items():
            args[at] = v
        with pytest.raises(lib.FiberHipError):
            lib.call("fiber_det_merge", *args)
    lib.call("fiber_det_merge", *([None] * 12), 0, K, D, Cc, 1)          # B == 0
    lib.call("fiber_det_merge", *([None] * 12), 3, 0, D, Cc, 0)          # K * D == 0
    torch.cuda.synchronize()


# ---- the split forward ---------------------------------------------------------------------------------------------------------------------
def _tok(prompts, rows):
    return {"input_ids": prompts.input_ids[rows], "attention_mask": prompts.attention_mask[rows]}


@pytest.mark.parametrize("which", ["shallow", "deep"])
def test_split_forward_is_the_unsplit_forward_bit_for_bit(which, request, prompts):
    model = request.getfixturevalue(which)
    fb = model.fusion_backbone
    images, _ = cc.pair_inputs(DEV)
    tok = _tok(prompts, torch.tensor([0, 2], device=DEV))
    with torch.no_grad():
        old = cc.named(*cc.forward_unsplit(fb, tok, images)[:2])
        ist, tst = fb.image_prefix(images), fb.text_prefix(tok)
        assert (ist.stage, ist.block) == ((3, 0) if which == "shallow" else (2, 14))
        split_v, split_l, _ = fb.fuse(ist, tst)
        again_v, _, _ = fb.fuse(ist, tst)                    # the states are not consumed
        new_v, new_l, _ = fb(tok, images)
    for name, want in old.items():
        for got in (cc.named(split_v, split_l)[name], cc.named(new_v, new_l)[name]):
            assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), f"{which}: {name}"
    assert all(torch.equal(a, b) for a, b in zip(split_v, again_v))
    assert set(new_l) == {"aggregate", "embedded", "masks", "hidden"} and float(old["p3"].abs().sum()) > 0


def test_pair_batch_against_the_replicated_batch(deep, prompts):
    """fuse on gathered rows (the prefixes computed once, at batch B and K) against the existing forward on the explicitly replicated
    batch (the prefixes computed at batch B * p): equal, or within GPU_FACTOR times the forward's own measured sensitivity to the batch it
    runs in (chunk_cases.BATCH_SENSITIVITY)."""
    fb = deep.fusion_backbone
    images, _ = cc.pair_inputs(DEV)
    B, P = cc.PAIR["B"], cc.PAIR["P"]
    assert cc.BATCH_SENSITIVITY is not None and cc.passes(len(prompts), P) == [(0, 2), (2, 1)]
    with torch.no_grad():
        ist, tst = fb.image_prefix(images), fb.text_prefix(_tok(prompts, slice(None)))
        for k0, p in cc.passes(len(prompts), P):
            ii, ti = cc.pair_indices(B, k0, p, DEV)
            got = cc.named(*fb.fuse(ist, tst, ii, ti)[:2])
            want = cc.named(*fb(_tok(prompts, ti), images.repeat_interleave(p, 0))[:2])
            for name, w in want.items():
                d, s = fc.rel_l2(got[name], w), cc.BATCH_SENSITIVITY[name]
                print(f"pass ({k0}, {p}) {name}: rel-L2 {d:.3e}, measured sensitivity {s:.3e}")
                assert got[name].shape == w.shape
                if s == 0:
                    assert torch.equal(got[name], w), f"pass ({k0}, {p}): {name}"
                else:
                    assert d <= fc.GPU_FACTOR * s, f"pass ({k0}, {p}): {name}: {d} > {fc.GPU_FACTOR} x {s}"


# ---- detect_chunked against the existing head, pair by pair ------------------------------------------------------------------------------------
class HeadTape:
    """The two one-channel 1 x 1 convolutions of VLDyHead (cls_logits, centerness; nn.Conv2d) do not give the same last bit twice on the
    same input at the finest level, so two executions of the head cannot be compared with torch.equal (profiles/chunked_detection.md).
    The tape records what the head returned for each call and, played back, hands the same tensors to the next run's calls in order,
    after checking (check=True) that the features it was called with are the recorded ones bit for bit.  Everything around the head --
    the pair-batch layout, the gathered maps, the chunk width, the post-processor, the merge -- runs again."""

    def __init__(self, head):
        self.calls, self.queue, self.check = [], None, True
        self.handle = head.register_forward_hook(self)

    def __call__(self, module, args, output):
        if self.queue is None:
            self.calls.append((args[0], args[1]["embedded"], output))
            return None
        features, embedded, recorded = self.queue.pop(0)
        if self.check:
            assert len(features) == len(args[0]) and all(torch.equal(a, b) for a, b in zip(features, args[0])), "the head's features differ"
            assert torch.equal(embedded, args[1]["embedded"])
        return recorded

    def play(self, check=True):
        self.queue, self.check = list(self.calls), check

    def close(self):
        self.handle.remove()


@pytest.fixture
def tape(shallow):
    t = HeadTape(shallow.rpn.head)
    yield t
    t.close()


def _per_chunk(model, images, sizes, prompts, P):
    """The features detect_chunked computes for each pass, through the existing model.rpn with one positive-map dict per sample and the
    chunk width -> (boxes [B, K, D, 4], scores, labels, source [B, K, D], count [B, K]) on the host"""
    fb, B, K, Cc = model.fusion_backbone, images.shape[0], len(prompts), prompts.chunk_width
    cols = []
    with torch.no_grad():
        ist = fb.image_prefix(images)
        tst = fb.text_prefix({"input_ids": prompts.input_ids, "attention_mask": prompts.attention_mask})
        for k0, p in cc.passes(K, P):
            ii, ti = cc.pair_indices(B, k0, p, DEV)
            visual, lang, _ = fb.fuse(ist, tst, ii, ti)
            maps = [prompts.positive_maps[k0 + j] for _ in range(B) for j in range(p)]
            det = model.rpn([sizes[b] for b in range(B) for _ in range(p)], list(visual), lang, maps, None, num_classes=Cc)
            assert det.boxes.shape == (B * p, det.scores.shape[1], 4)
            cols.append([t.view(B, p, *t.shape[1:]).cpu() for t in (det.boxes, det.scores, det.labels, det.source, det.count)])
    return tuple(torch.cat(c, dim=1) for c in zip(*cols))


def _host_merged(cols, prompts, max_dets):
    """merged by the list reference -> Detections on the device"""
    from fiber_amd.modules import Detections
    *merged, chunk, total = cc.merge_ref(*cols, prompts.label_table.cpu(), max_dets)
    return Detections(*(t.to(DEV) for t in merged), total.to(DEV), chunk=chunk.to(DEV))


@pytest.mark.parametrize("P,max_dets", [(2, None), (1, 7), (None, 100)])
def test_detect_chunked_equals_the_head_pair_by_pair(shallow, prompts, tape, P, max_dets):
    images, sizes = cc.pair_inputs(DEV)
    state = shallow.encode_prompts(prompts)
    got = shallow.detect_chunked((images, sizes), state, prompts_per_pass=P, max_dets=max_dets)
    assert len(tape.calls) == len(cc.passes(len(prompts), P or len(prompts)))
    tape.play()
    cols = _per_chunk(shallow, images, sizes, prompts, P or len(prompts))
    assert tape.queue == []
    want = _host_merged(cols, prompts, max_dets)
    K, D = len(prompts), shallow.cfg.MODEL.ATSS.DETECTIONS_PER_IMG
    assert got.scores.shape == (2, K * D if max_dets is None else min(max_dets, K * D))
    for field in ("boxes", "scores", "labels", "source", "count", "chunk"):
        g, w = getattr(got, field), getattr(want, field)
        assert g.dtype == w.dtype and torch.equal(g, w), field
    assert int((cols[4] > 0).sum()) >= 4, cols[4]              # (several chunks have something to merge)
    live = got.labels[got.scores >= 0]
    assert int(live.min()) >= 1 and int(live.max()) <= 5 and live.unique().numel() > 2
    assert bool((got.chunk[got.scores >= 0] == (got.labels[got.scores >= 0] - 1) // 2).all())      # label_table: chunks of two


def test_detect_chunked_refusals(shallow, prompts):
    images, sizes = cc.pair_inputs(DEV)
    state = shallow.encode_prompts(prompts)
    with pytest.raises(ValueError, match="prompts_per_pass"):
        shallow.detect_chunked((images, sizes), state, prompts_per_pass=0)
    shallow.train()
    try:
        with pytest.raises(RuntimeError, match="training mode"):
            shallow.detect_chunked((images, sizes), state)
        with pytest.raises(RuntimeError, match="training mode"):
            shallow.encode_prompts(prompts)
    finally:
        shallow.eval()


# ---- the evaluation loop -------------------------------------------------------------------------------------------------------------------
def _batches(n):
    from fiber_amd.data import DetImageList
    g = np.random.default_rng(11)
    out = []
    for i in range(n):
        t = torch.from_numpy(g.standard_normal((2, 3, cc.PAIR["H"], cc.PAIR["W"])).astype(np.float32)).to(DEV)
        out.append(DetImageList(t, list(cc.PAIR["sizes"]), [(128, 192, 0), (90, 135, 0)]))
    return out


def _ground_truth(images, det, cats, first_id):
    """every third detection of an image, grown by a pixel in its original frame, is a ground truth of its category"""
    hb, hl, hc = images.boxes_to_original(det).cpu().numpy(), det.labels.cpu().numpy(), det.count.cpu().numpy()
    samples = []
    for b in range(hb.shape[0]):
        anns = []
        for i in range(0, int(hc[b]), 3):
            x1, y1, x2, y2 = [float(v) for v in hb[b, i]]
            if x2 - x1 > 1 and y2 - y1 > 1:
                w, h = float(np.ceil(x2 - x1)) + 1, float(np.ceil(y2 - y1)) + 1
                anns.append(dict(bbox=[float(np.floor(x1)), float(np.floor(y1)), w, h], area=w * h, category_id=cats[int(hl[b, i]) - 1]["id"]))
        present = {a["category_id"] for a in anns}
        samples.append(dict(image_id=first_id + b, annotations=anns, neg_category_ids=[c["id"] for c in cats[:2] if c["id"] not in present],
                            not_exhaustive_category_ids=[]))
    return samples


@pytest.mark.parametrize("kind", [dict(max_dets=4), dict(fixed_ap_topk=3)])
def test_evaluate_detection_chunked(shallow, prompts, tape, kind):
    from fiber_amd.modules import BoxAPEvaluator, evaluate_detection_chunked, pack_detection_targets
    cats = cc.PAIR["categories"]
    ref = BoxAPEvaluator(cats, **kind)
    cut = ref.max_dets if ref.max_dets >= 0 else None
    fed = []
    for n, images in enumerate(_batches(2)):
        cols = _per_chunk(shallow, images.tensors, images.image_sizes, prompts, cc.PAIR["P"])
        targets = pack_detection_targets(_ground_truth(images, _host_merged(cols, prompts, None), cats, 2 * n), cats).to(DEV)
        det = _host_merged(cols, prompts, cut)
        ref.update(det, targets, boxes=images.boxes_to_original(det))
        fed.append({"images": images, "targets": targets})
    want = ref.summarize()
    assert want["AP"] > 0 and int(ref.num_gt.sum()) > 0 and len(tape.calls) == 4
    ev = BoxAPEvaluator(cats, **kind)
    tape.play()
    first = evaluate_detection_chunked(shallow, fed, ev, prompts, prompts_per_pass=cc.PAIR["P"])      # (also: every lazily built table now exists)
    assert list(first) == list(want) and [float(v) for v in first.values()] == [float(v) for v in want.values()] and tape.queue == []
    # again, with every synchronising call before summarize an error
    ev.reset()
    mode, summarize = torch.cuda.get_sync_debug_mode(), ev.summarize

    def leave_then_summarize():
        torch.cuda.set_sync_debug_mode(mode)
        return summarize()
    ev.summarize = leave_then_summarize
    tape.play(check=False)                                   # (the tape's own comparisons would synchronise)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = evaluate_detection_chunked(shallow, fed, ev, prompts, prompts_per_pass=cc.PAIR["P"])
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert [float(v) for v in again.values()] == [float(v) for v in want.values()]


def test_evaluate_detection_chunked_at_lvis_width(shallow):
    """1203 categories: 31 prompts of 40, eight per pass.  One prompt of 1203 names does not fit in 256 tokens, and 1203 (or the
    reference's 3000) classes do not fit the decode kernel's 10-bit class field: the chunked loop is the only way through."""
    from fiber_amd.modules import BoxAPEvaluator, build_detection_prompts, evaluate_detection_chunked, pack_detection_targets
    cats = [dict(id=3 * i + 7, name=f"thing{i} kind", frequency="rcf"[i % 3]) for i in range(1203)]
    lvis = build_detection_prompts(cats, cc.StubTokenizer(), chunk=40).to(DEV)
    assert len(lvis) == 31 and lvis.chunk_width == 40
    images = _batches(1)[0]
    state = shallow.encode_prompts(lvis)
    det = shallow.detect_chunked(images, state, prompts_per_pass=8, max_dets=300)
    assert det.scores.shape == (2, 300) and int(det.count.min()) > 0 and int(det.labels.max()) <= 1203
    assert det.labels[det.scores >= 0].unique().numel() > 40 and det.chunk[det.scores >= 0].unique().numel() > 1
    live = det.scores >= 0
    assert bool((det.chunk[live] == (det.labels[live] - 1) // 40).all()) and bool((det.scores[:, :-1] >= det.scores[:, 1:]).all())
    targets = pack_detection_targets(_ground_truth(images, det, cats, 0), cats).to(DEV)
    ev = BoxAPEvaluator(cats, max_dets=300)
    res = evaluate_detection_chunked(shallow, [{"images": images, "targets": targets}], ev, lvis, prompts_per_pass=8)
    assert set(res) >= {"AP", "AP50", "APr", "APc", "APf", "AR@300"} and all(math.isfinite(float(v)) for v in res.values())
    assert res["AP"] > 0
