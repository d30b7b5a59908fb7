"""Cases and scalar restatement of phrase-grounding evaluation (fiber_amd/modules/grounding_eval.py, csrc/geval.hip).

`restate` is the device-independent yardstick: both modes of fiber_ground_recall written out one number at a time on numpy scalars (fp64
IoU for Flickr recall, fp32 generalized IoU for RefExp precision, every operation rounded once in the reference's order), straight from
the sample lists.  It shares no code with the package: it merges boxes, ranks detections and indexes categories itself.
tests/test_ground_eval_host.py holds it and the package's CPU path against fixtures the reference's own evaluators produced
(tools/gen_ground_eval_golden.py: inputs by name from here, the fixtures hold outputs only); tests/test_hip_ground_eval.py holds the
kernel against both.

Cases (the smallest shapes at which the kernel can still go wrong; D = 100 = one full chunk of 64 and a partial one):
  geval_flickr_small  B = 3, counts (100, 37, 0), P <= 5, G <= 3, topk (1, 5, 10, -1).
                      image 0: phrase 0 first hit at rank 0; phrase 1 at rank 4 (@1 misses, @5 hits); phrase 2 at rank 5 (@5 misses, @10
                      hits) with ranks 0-3 at positions below 64 and ranks 4-6 above (the rank carry across the chunk boundary);
                      phrase 3 has detections only past position 64; phrase 4 has 3 detections (fewer than 5), two types, two gt boxes
                      of which only the second is matched.
                      image 1: phrase 0 has no detection (the sentinel alone is ranked); phrase 1 sits at IoU = 1/2 EXACTLY
                      ([0, 0, 10, 10] against [0, 0, 10, 20]; every intermediate is a small integer), which pins >=; phrase 2 first
                      hit at rank 7; phrase 3 has three gt boxes and misses; row 4 is padding (gt_count 0).  Rows 37..99 hold boxes
                      that WOULD hit phrase 0: reading past count shows.
                      image 2: no detection at all; every row is such a trap.
  geval_flickr_merge  the same with merge_boxes=True.
  geval_refexp        B = 4, counts (100, 64, 1, 0), topk (1, 5, 10), three dataset names; image 0 hits only at rank 7; image 1 at
                      rank 0; image 2's one box is disjoint from its target (negative GIoU); image 3 has no detection.  Targets are
                      xywh with values fp32 cannot hold, converted as the reference does ([x, y, w + x, h + y] in double).
  geval_maps          B = 3 per-sample positive maps for C = 6 (sample 0 of a B = 2 case repeated as sample 2, so that one image is scored
                      under two captions): one map leaves class 5 unused and has a single-token class, one uses two classes only, one
                      uses all six.  The score kernel and the post-processor run them on detect_small's head outputs, the end-to-end
                      test on the ground_small head inputs and weights.

Margins the generator asserts (conditions on the inputs, not measurements): every best differs from the threshold by >= MARGINS[mode]
except the phrases listed in EXACT, and no two detections of an image share a score.
"""
import types

import numpy as np

from oracle import detgen

D = 100
FRAME = (640, 480)                                           # (w, h) of every synthetic image
FLICKR_TOPK = (1, 5, 10, -1)
REFEXP_TOPK = (1, 5, 10)
THRESH = 0.5
FLICKR_CATEGORIES = ("people", "clothing", "bodyparts", "animals", "vehicles", "instruments", "scene", "other")
REFEXP_DATASETS = ("refcoco", "refcoco+", "refcocog")
MARGINS = {0: 1e-6, 1: 1e-4}
EXACT = {"geval_flickr_small": [(1, 1)], "geval_flickr_merge": [(1, 1)], "geval_refexp": []}     # (image, phrase) at best == thresh
CASES = {"geval_flickr_small": dict(mode=0, merge=False, seed=0), "geval_flickr_merge": dict(mode=0, merge=True, seed=0),
         "geval_refexp": dict(mode=1, merge=False, seed=0)}

# image -> phrases: gt boxes (integers, as the Flickr xml holds them), types, the positions (indices into the score-ordered detections) of
# the phrase's detections and the ranks among them that are built to match gt box `on`.  fill: the label every other position gets.
_FLICKR = [
    dict(id="1001", count=100, fill=(1, 2), phrases=[
        dict(gt=[[40, 60, 200, 300]], types=["people"], pos=[0, 3, 9], hits={0: 0}),
        dict(gt=[[250, 40, 420, 200]], types=["clothing"], pos=[1, 4, 10], hits={4: 0}),
        dict(gt=[[60, 320, 260, 460]], types=["animals"], pos=[2, 5, 11, 22, 70, 71, 90], hits={5: 0}),
        dict(gt=[[450, 250, 600, 440]], types=["vehicles"], pos=[69, 80, 95], hits={1: 0}),
        dict(gt=[[300, 230, 380, 330], [480, 30, 620, 180]], types=["people", "clothing"], pos=[6, 40, 99], hits={2: 1}),
    ]),
    dict(id="1002", count=37, fill=(3,), phrases=[
        dict(gt=[[100, 100, 300, 260]], types=["scene"], pos=[], hits={}),
        dict(gt=[[0, 0, 10, 20]], types=["other"], pos=[0, 8, 20], hits={}, exact=[0.0, 0.0, 10.0, 10.0]),
        dict(gt=[[330, 200, 560, 420]], types=["people"], pos=None, hits={7: 0}),
        dict(gt=[[20, 300, 120, 400], [150, 300, 250, 400], [50, 420, 200, 470]], types=["bodyparts", "other"], pos=[3, 13, 30], hits={}),
    ]),
    dict(id="1003", count=0, fill=(1,), phrases=[
        dict(gt=[[100, 80, 400, 380]], types=["people"], pos=[], hits={}),
        dict(gt=[[10, 10, 90, 200], [500, 300, 630, 470]], types=["instruments"], pos=[], hits={}),
    ]),
]
# what the layout above is built to give: (image, phrase) -> hit at topk (1, 5, 10, -1), without merging
FLICKR_EXPECT = {(0, 0): (1, 1, 1, 1), (0, 1): (0, 1, 1, 1), (0, 2): (0, 0, 1, 1), (0, 3): (0, 1, 1, 1), (0, 4): (0, 1, 1, 1),
                 (1, 0): (0, 0, 0, 0), (1, 1): (1, 1, 1, 1), (1, 2): (0, 0, 1, 1), (1, 3): (0, 0, 0, 0), (2, 0): (0, 0, 0, 0), (2, 1): (0, 0, 0, 0)}

_REFEXP = [
    dict(id=11, count=100, dataset="refcoco", xywh=[100.1, 50.3, 200.7, 150.9], hits=[7]),
    dict(id=12, count=64, dataset="refcoco+", xywh=[300.2, 200.6, 120.3, 180.1], hits=[0, 30]),
    dict(id=13, count=1, dataset="refcocog", xywh=[20.7, 30.9, 100.3, 80.1], hits=[], disjoint=True),
    dict(id=14, count=0, dataset="refcoco", xywh=[200.3, 100.7, 150.1, 120.9], hits=[]),
]
REFEXP_EXPECT = {0: (0, 0, 1), 1: (1, 1, 1), 2: (0, 0, 0), 3: (0, 0, 0)}


def _f32(v):
    return np.asarray(v, dtype=np.float32)


def _near(g, box, lo, hi):
    """`box` with every edge moved by a non-integer amount of magnitude in [lo, hi)"""
    return _f32(np.asarray(box, dtype=np.float64) + g.uniform(lo, hi, 4) * g.choice([-1.0, 1.0], 4))


def _shifted(g, box):
    """`box` moved sideways or up by 55..90 % of its extent (IoU with it below 0.3), clipped to the frame"""
    x1, y1, x2, y2 = [float(v) for v in box]
    w, h = x2 - x1, y2 - y1
    f = g.uniform(0.55, 0.9) * g.choice([-1.0, 1.0])
    dx, dy = (f * w, g.uniform(-0.1, 0.1) * h) if g.random() < 0.5 else (g.uniform(-0.1, 0.1) * w, f * h)
    b = np.array([x1 + dx, y1 + dy, x2 + dx, y2 + dy]) + g.uniform(-2.0, 2.0, 4)
    b[[0, 2]] = b[[0, 2]].clip(0, FRAME[0] - 1)
    b[[1, 3]] = b[[1, 3]].clip(0, FRAME[1] - 1)
    return _f32(b)


def _scores(g, B):
    s = 0.97 - 0.009 * np.arange(D)[None, :] + g.uniform(0.0, 0.004, (B, D))
    return _f32(s)


def flickr_detections(case="geval_flickr_small"):
    """-> SimpleNamespace(boxes fp32 [B, D, 4] in the original frame, scores fp32 [B, D], labels int32 [B, D], count int32 [B]): numpy,
    seeded by name.  Rows past count carry score -1 and a box that would hit phrase 0."""
    g = detgen._rng("geval:flickr", CASES[case]["seed"])
    B = len(_FLICKR)
    boxes, labels = np.zeros((B, D, 4), np.float32), np.zeros((B, D), np.int32)
    scores = _scores(g, B)
    for b, im in enumerate(_FLICKR):
        n = im["count"]
        lab = np.zeros(D, np.int64)
        for p, ph in enumerate(im["phrases"]):
            if ph["pos"]:
                lab[ph["pos"]] = p + 1
        free = [i for i in range(n) if lab[i] == 0]
        for j, i in enumerate(free):
            lab[i] = im["fill"][j % len(im["fill"])]
        for p, ph in enumerate(im["phrases"]):
            mine = [i for i in range(n) if lab[i] == p + 1]
            for r, i in enumerate(mine):
                if r in ph["hits"]:
                    boxes[b, i] = _near(g, ph["gt"][ph["hits"][r]], 0.5, 4.0)
                elif "exact" in ph:
                    boxes[b, i] = _f32(ph["exact"]) if r == 0 else _f32([400 + 17.5 * r, 300 + 3.25 * r, 460 + 17.5 * r, 390 + 3.25 * r])
                else:
                    boxes[b, i] = _shifted(g, ph["gt"][int(g.integers(len(ph["gt"])))])
        lab[n:] = 1
        boxes[b, n:] = _f32(im["phrases"][0]["gt"][0])
        scores[b, n:] = -1.0
        labels[b] = lab
    return types.SimpleNamespace(boxes=boxes, scores=scores, labels=labels, count=np.array([im["count"] for im in _FLICKR], np.int32))


def flickr_samples():
    """The ground truth as pack_phrase_targets takes it (and as the generator writes it into a Flickr-layout directory)."""
    return [dict(image_id=im["id"], sentence_id=0,
                 phrases=[dict(boxes=[list(bx) for bx in ph["gt"]], phrase_type=list(ph["types"])) for ph in im["phrases"]]) for im in _FLICKR]


def refexp_xyxy(xywh):
    """refexp.py:63-69: [x, y, w + x, h + y] in double"""
    return [xywh[0], xywh[1], xywh[2] + xywh[0], xywh[3] + xywh[1]]


def refexp_detections(case="geval_refexp"):
    g = detgen._rng("geval:refexp", CASES[case]["seed"])
    B = len(_REFEXP)
    boxes, labels = np.zeros((B, D, 4), np.float32), np.ones((B, D), np.int32)
    scores = _scores(g, B)
    for b, im in enumerate(_REFEXP):
        n, t = im["count"], refexp_xyxy(im["xywh"])
        for i in range(n):
            if im.get("disjoint"):
                boxes[b, i] = _f32([400.5, 300.25, 520.75, 410.5])
            elif i in im["hits"]:
                boxes[b, i] = _near(g, t, 0.5, 4.0)
            else:
                boxes[b, i] = _shifted(g, t)
        boxes[b, n:] = _f32(t)
        scores[b, n:] = -1.0
    return types.SimpleNamespace(boxes=boxes, scores=scores, labels=labels, count=np.array([im["count"] for im in _REFEXP], np.int32))


def refexp_samples():
    return [dict(image_id=im["id"], sentence_id=0, dataset_name=im["dataset"], bbox_xywh=list(im["xywh"]),
                 phrases=[dict(boxes=[refexp_xyxy(im["xywh"])], phrase_type=[])]) for im in _REFEXP]


def case_inputs(case):
    """-> (detections, samples, categories, topk, mode, merge)"""
    c = CASES[case]
    if c["mode"] == 0:
        return flickr_detections(case), flickr_samples(), FLICKR_CATEGORIES, FLICKR_TOPK, 0, c["merge"]
    return refexp_detections(case), refexp_samples(), REFEXP_DATASETS, REFEXP_TOPK, 1, False


# ---- the restatement: one number at a time ----------------------------------------------------------------------------------------------
def iou64(a, t):
    """flickr_eval.py:173-204 on one pair of np.float64 boxes"""
    area1 = (a[2] - a[0]) * (a[3] - a[1])
    area2 = (t[2] - t[0]) * (t[3] - t[1])
    w = max(min(a[2], t[2]) - max(a[0], t[0]), np.float64(0))
    h = max(min(a[3], t[3]) - max(a[1], t[1]), np.float64(0))
    inter = w * h
    return inter / (area1 + area2 - inter)


def giou32(a, t):
    """set_loss.py:15-52 on one pair of np.float32 boxes"""
    zero = np.float32(0)
    area1 = (a[2] - a[0]) * (a[3] - a[1])
    area2 = (t[2] - t[0]) * (t[3] - t[1])
    w = max(min(a[2], t[2]) - max(a[0], t[0]), zero)
    h = max(min(a[3], t[3]) - max(a[1], t[1]), zero)
    inter = w * h
    union = area1 + area2 - inter
    iou = inter / union
    cw = max(max(a[2], t[2]) - min(a[0], t[0]), zero)
    ch = max(max(a[3], t[3]) - min(a[1], t[1]), zero)
    area = cw * ch
    return iou - (area - union) / area


def restate(boxes, labels, count, samples, topk, thresh, mode, merge=False):
    """boxes [B, D, 4] fp32, labels [B, D], count [B] (numpy); samples as pack_phrase_targets takes them.
    -> dict(hit int32 [B, P, K], best fp64 [B, P, K] (0 in padding rows), positives / totals {k: {category: n}})"""
    B = len(samples)
    P = max([len(s["phrases"]) for s in samples] + [1])
    K = len(topk)
    hit, best = np.zeros((B, P, K), np.int32), np.zeros((B, P, K), np.float64)
    pos, tot = {k: {} for k in topk}, {k: {} for k in topk}
    for b, s in enumerate(samples):
        n = int(count[b])
        for p, ph in enumerate(s["phrases"]):
            gts = [[np.float64(v) for v in bx] for bx in ph["boxes"]]
            if merge and len(gts) > 1:
                gts = [[min(t[0] for t in gts), min(t[1] for t in gts), max(t[2] for t in gts), max(t[3] for t in gts)]]
            if mode == 0:
                ranked = [[np.float64(v) for v in boxes[b, i]] for i in range(n) if int(labels[b, i]) == p + 1]
                ranked.append([np.float64(0)] * 4)
                vals = [max(iou64(a, t) for t in gts) for a in ranked]
                thr = np.float64(thresh)
            else:
                ranked = [[np.float32(v) for v in boxes[b, i]] for i in range(n)]
                gts = [[np.float32(v) for v in t] for t in gts]
                vals = [max(giou32(a, t) for t in gts) for a in ranked]
                thr = np.float32(thresh)
            cats = ["all"] + sorted(set(ph.get("phrase_type", []))) + ([s["dataset_name"]] if s.get("dataset_name") else [])
            for j, k in enumerate(topk):
                seen = vals if k < 0 else vals[:k]
                m = max(seen) if seen else np.float64(-1)
                h = bool(seen) and bool(m >= thr)
                hit[b, p, j], best[b, p, j] = int(h), float(m)
                for c in cats:
                    tot[k][c] = tot[k].get(c, 0) + 1
                    pos[k][c] = pos[k].get(c, 0) + int(h)
    return dict(hit=hit, best=best, positives=pos, totals=tot)


def report(r):
    """RecallTracker.report of a restatement"""
    return {k: {c: r["positives"][k][c] / n for c, n in r["totals"][k].items()} for k in r["totals"]}


def tables(r, categories, topk):
    """The restatement's counts in the kernel's layout: (positives, totals) int64 [K, 64] with "all" at column 0"""
    cats = ["all"] + [c for c in categories if c != "all"]
    pos, tot = np.zeros((len(topk), 64), np.int64), np.zeros((len(topk), 64), np.int64)
    for j, k in enumerate(topk):
        for c, n in r["totals"][k].items():
            tot[j, cats.index(c)] = n
            pos[j, cats.index(c)] = r["positives"][k][c]
    return pos, tot


def refexp_results(r, datasets, topk):
    """RefExpEvaluator.summarize of a restatement: {dataset: sorted precisions}, 0.0 for a dataset without images"""
    out = {}
    for d in datasets:
        out[d] = sorted((r["positives"][k].get(d, 0) / r["totals"][k][d]) if r["totals"][k].get(d) else 0.0 for k in topk)
    return out


def ulp(x, dtype):
    return np.spacing(np.abs(np.asarray(x, dtype=dtype))).astype(np.float64)


# ---- per-sample positive maps on the ground_small head inputs ----------------------------------------------------------------------------
MAPS_C = 6
MAPS = [{1: [3, 4, 5], 2: [5, 6], 3: [17], 4: [30, 31, 32, 33, 200], 6: [4, 31, 90]},        # class 5 unused, class 3 a single token
        {1: [7], 2: [8, 9, 10]},                                                              # two classes only
        {1: [40, 41], 2: [42], 3: [43, 44, 45], 4: [3], 5: [100, 101], 6: [200, 255]}]


def three(t):
    """[2, ...] -> [3, ...]: sample 0 repeated as sample 2 (the ground_small / detect_small inputs have B = 2)"""
    import torch
    return torch.cat([t, t[:1]], dim=0).contiguous()
