"""Cases and scalar restatement of COCO-protocol box AP (fiber_amd/modules/detection_eval.py: CocoBoxEvaluator, csrc/apeval.hip:
fiber_ap_match_coco).

PARITY UNPINNED against the pycocotools binary: the library is neither in the reference tree nor available here, so no fixture holds
COCOeval's own output.  `restate` is the yardstick instead: evaluateImg / accumulate / summarize written out one number at a time on numpy
fp64 scalars in the COCO API's own loop form (sorted ground truths, a running best IoU, `break` at the first ignored one after a
non-ignored match), straight from the sample lists.  It shares no code with the package: it groups, sorts, caps, matches and accumulates
itself.  The cases are addressed by name so that a fixture generator can be added where pycocotools exists.

Cases (the smallest shapes at which each piece can still go wrong):
  coco_small  6 images, 5 categories, 0-5 ground truths (about one in five crowd) and 8 detections per image.  Fed as one update and as
              two updates of 3 images.
  coco_crowd  hand-worked, plus_one = 0, one category and one image per item (categories 11..16, images 0..5); T = 10 thresholds
              t0 = 0.50 .. t9 = 0.95, area ranges a0 all, a1 small, a2 medium, a3 large; a word's bit is a * 10 + t.  See CROWD_BITS:
              (a) image 0: a 200 x 200 crowd box and two detections inside it (crowd IoU 1): both match it at every (a, t) and both are
                  ignored everywhere.  A third, lower-scoring detection sits exactly on a normal 50 x 50 ground truth (area 2500:
                  medium): with the first two ignored, not false positives, the category's precision at a0 is 1 / (1 + 2^-52) at every recall,
                  not 1 / 3.
              (b) image 1: a 10 x 10 detection inside a 100 x 100 crowd region: crowd IoU exactly 1 (plain IoU would be 0.01): matched
                  and ignored at every (a, t).
              (c) image 2: a 100 x 100 detection, a normal 100 x 62 ground truth inside it (IoU 0.62, area 6200: medium) and a crowd
                  region around both (crowd IoU 1).  a0 and a2: matched at every t; the normal one wins at t0..t2 (not ignored), from
                  t3 = 0.65 up only the crowd qualifies (ignored, not a false positive).  a1 and a3: the normal one is out of range,
                  both are ignored and the crowd's larger IoU wins: ignored at every t.
              (d) image 3: a ground truth with `ignore: 1, iscrowd: 0` (40 x 40, medium) and a detection exactly on it: num_gt counts it
                  (1 at a0 and a2), matched at every (a, t), ignored only where the area range excludes it (a1, a3).
              (e) image 4: two 40 x 40 ground truths at bit-equal IoU 7/9 to the first detection: the LATER one is taken (t0..t5); the
                  second detection then gets the earlier one at 0.8605 (t0..t7; the other way round it would have 0.702, t0..t4).  All
                  medium: in a1 and a3 everything is ignored.
              (f) image 5: a 10 x 10 detection inside a 20 x 10 ground truth, IoU = 1/2 EXACTLY (every intermediate a small integer):
                  matched at t0 only.  Ground truth (200) and detection (100) are small: in a2 and a3 ignored at every t.
  coco_cap    max_dets (1, 10, 100), run with plus_one = 1 and 0; categories 5, 9, 13:
              image 0: 103 detections of category 5 interleaved in score order with 12 of category 9.  Category 5 has a ground truth on
                  its best detection and one that only its detection of rank 101 covers (IoU 1 with plus_one): that slot is cut
                  (valid 0, words 0) and the ground truth stays unmatched.  Category 9 has 12 ground truths and 12 detections, each a
                  true positive: recall 1/12, 10/12 and 1 at max_dets 1, 10, 100.
              image 1: category 13, a 19 x 9.5 detection inside a 20 x 20 ground truth: IoU 0.45125 without and 0.525 with plus_one, so
                  bit t0 of a0 differs between the two settings.  A few more detections of the other categories (category 9 has no ground
                  truth here: a false positive).
  coco_wide   max_dets (1, 10, 100, 300): image 0: 70 ground truths of category 1, three of them crowd at annotation indices 64, 66 and
              69 (the second chunk of 64 lanes), and 200 detections; image 1: 30 more.  230 records > 3 * fiber_ap_chunk() at the last
              rung, which is why the ladder has a fourth rung here: at 100 only 130 exist.
  coco_lvis_identity  the inputs of det_eval_cases' apeval_small with the ignore flags removed, plus_one = 0, max_dets (300,).  With every
              category in every image's negative list and an empty not-exhaustive list the LVIS protocol coincides with the COCO one,
              and only there: CocoBoxEvaluator's num_gt and tables must equal BoxAPEvaluator(max_dets=300)'s, which the reference's own
              LVISEval fixtures pin.  lvis_side() gives the LVIS samples; no image has 300 detections or more.

Conditions the generator asserts on the inputs (not measurements): every IoU of a same-category pair in an image (under the crowd rule for
a crowd ground truth, under every plus_one setting the case runs with) differs from every threshold by >= MARGIN except the pairs in
EXACT, which must equal it; no two detections of one category share a score over the case.
"""
import types

import numpy as np

import det_eval_cases as dv
from oracle import detgen

MARGIN = 1e-6
IOU_THRS = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
REC_THRS = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
AREA_RNG = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)
T, A = len(IOU_THRS), len(AREA_RNG)
CASES = {"coco_small": dict(seed=0, max_dets=(1, 10, 100), plus_one=(1,)), "coco_crowd": dict(seed=0, max_dets=(1, 10, 100), plus_one=(0,)),
         "coco_cap": dict(seed=0, max_dets=(1, 10, 100), plus_one=(1, 0)), "coco_wide": dict(seed=0, max_dets=(1, 10, 100, 300), plus_one=(1,)),
         "coco_lvis_identity": dict(seed=0, max_dets=(300,), plus_one=(0,))}
RUNS = [(case, p) for case, spec in CASES.items() for p in spec["plus_one"]]
EXACT = {"coco_small": [], "coco_crowd": [(5, 0, 0, 0.5)], "coco_cap": [], "coco_wide": [], "coco_lvis_identity": []}      # (image, slot, annotation, IoU)
SMALL_CATEGORIES = [dict(id=3), dict(id=7), dict(id=8), dict(id=12), dict(id=20)]
CROWD_CATEGORIES = [dict(id=11 + i) for i in range(6)]
CAP_CATEGORIES = [dict(id=5), dict(id=9), dict(id=13)]
WIDE_CATEGORIES = [dict(id=1), dict(id=4)]
_cache = {}


def word(bits):
    """{area range: thresholds} -> the uint64 with bit a * T + t set"""
    w = 0
    for a, ts in bits.items():
        for t in ts:
            w |= 1 << (a * T + t)
    return np.uint64(w)


ALL_T = range(T)
EVERY = {a: ALL_T for a in range(A)}
# coco_crowd, by (image, slot): (match word, ignore word); slots are in descending score
CROWD_BITS = {(0, 0): (word(EVERY), word(EVERY)), (0, 1): (word(EVERY), word(EVERY)), (0, 2): (word(EVERY), word({1: ALL_T, 3: ALL_T})),
              (1, 0): (word(EVERY), word(EVERY)),
              (2, 0): (word(EVERY), word({0: range(3, T), 1: ALL_T, 2: range(3, T), 3: ALL_T})),
              (3, 0): (word(EVERY), word({1: ALL_T, 3: ALL_T})),
              (4, 0): (word({a: range(6) for a in range(A)}), word({1: ALL_T, 3: ALL_T})),
              (4, 1): (word({a: range(8) for a in range(A)}), word({1: ALL_T, 3: ALL_T})),
              (5, 0): (word({a: [0] for a in range(A)}), word({2: ALL_T, 3: ALL_T}))}
CROWD_NUM_GT = np.array([[1, 0, 1, 0], [0, 0, 0, 0], [1, 0, 1, 0], [1, 0, 1, 0], [2, 0, 2, 0], [1, 1, 0, 0]], dtype=np.int64)


def _ann(cat_id, xywh, area=None, iscrowd=0, ignore=None):
    a = dict(bbox=[float(v) for v in xywh], area=float(xywh[2] * xywh[3] if area is None else area), category_id=cat_id, iscrowd=iscrowd)
    if ignore is not None:
        a["ignore"] = ignore
    return a


def _small(seed):
    g = detgen._rng("cocoeval:small", seed)
    ids = [c["id"] for c in SMALL_CATEGORIES]
    per_image, samples, trap = [], [], []
    pool = list(dv._score_pool(g, 6 * 8 + 1))
    for b, ngt in enumerate([3, 0, 5, 2, 4, 1]):
        anns = []
        for _ in range(ngt):
            x, y, w, h = g.uniform(0, 400), g.uniform(0, 300), g.uniform(14, 180), g.uniform(14, 160)
            box = [round(float(x), 2), round(float(y), 2), round(float(w), 2), round(float(h), 2)]
            anns.append(_ann(ids[int(g.integers(len(ids)))], box, area=box[2] * box[3] * float(g.uniform(0.6, 1.0)),
                             iscrowd=1 if g.random() < 0.2 else 0, ignore=1 if g.random() < 0.15 else None))
        dets = []
        for k in range(8):
            if anns and k < 5:
                a = anns[int(g.integers(len(anns)))]
                label = ids.index(a["category_id"]) + 1 if g.random() < 0.85 else int(g.integers(len(ids))) + 1
                dets.append((dv._jitter(g, a["bbox"], [0.02, 0.06, 0.12, 0.2, 0.3][k]), pool.pop(), label))
            else:
                dets.append((dv._random_box(g), pool.pop(), int(g.integers(len(ids))) + 1))
        per_image.append(dets)
        samples.append(dict(image_id=100 + 7 * b, annotations=anns))
        trap.append((dv._jitter(g, anns[0]["bbox"], 0.0), ids.index(anns[0]["category_id"]) + 1) if anns else ([5, 5, 50, 50], 1))
    return dict(categories=SMALL_CATEGORIES, samples=samples, det=dv._pack(per_image, 12, trap))


def _crowd():
    c = [k["id"] for k in CROWD_CATEGORIES]
    im = [dict(anns=[_ann(c[0], [100, 100, 200, 200], iscrowd=1), _ann(c[0], [400, 100, 50, 50])],
               dets=[([110, 110, 150, 150], 0.9, 1), ([200, 200, 260, 270], 0.8, 1), ([400, 100, 450, 150], 0.3, 1)]),
          dict(anns=[_ann(c[1], [0, 0, 100, 100], iscrowd=1)], dets=[([20, 30, 30, 40], 0.7, 2)]),
          dict(anns=[_ann(c[2], [100, 100, 100, 62]), _ann(c[2], [50, 50, 300, 300], iscrowd=1)], dets=[([100, 100, 200, 200], 0.85, 3)]),
          dict(anns=[_ann(c[3], [300, 300, 40, 40], ignore=1)], dets=[([300, 300, 340, 340], 0.75, 4)]),
          dict(anns=[_ann(c[4], [200, 200, 40, 40]), _ann(c[4], [200, 210, 40, 40])],
               dets=[([200, 205, 240, 245], 0.97, 5), ([200, 203, 240, 243], 0.66, 5)]),
          dict(anns=[_ann(c[5], [300, 300, 20, 10])], dets=[([300, 300, 310, 310], 0.73, 6)])]
    samples = [dict(image_id=10 + b, annotations=x["anns"]) for b, x in enumerate(im)]
    trap = [([400, 100, 450, 150], 1), ([20, 30, 30, 40], 2), ([100, 100, 200, 200], 3), ([300, 300, 340, 340], 4), ([200, 200, 240, 240], 5),
            ([300, 300, 320, 310], 6)]
    return dict(categories=CROWD_CATEGORIES, samples=samples, det=dv._pack([x["dets"] for x in im], 4, trap))


def _cap(seed):
    g = detgen._rng("cocoeval:cap", seed)
    c = [k["id"] for k in CAP_CATEGORIES]
    pool = sorted(dv._score_pool(g, 140).tolist())           # ascending: pop() hands out the best first
    anns = [_ann(c[0], [10, 10, 30, 30]), _ann(c[0], [560, 400, 60, 60])]
    dets = [([10, 10, 39, 39], pool.pop(), 1)]               # the best detection of category 5: IoU 1 with plus_one
    rest = list(g.permutation(102 + 12))                     # the interleaving of the two categories in score order
    twelve = sorted(rest[:12])
    k5 = 0
    k9 = 0
    for i in range(102 + 12):
        if i in twelve:                                      # category 9: 12 ground truths on a row, each with its own detection
            x, y = 10 + 45 * k9, 420
            anns.append(_ann(c[1], [x, y, 40, 40]))
            dets.append(([x, y, x + 39, y + 39], pool.pop(), 2))
            k9 += 1
        else:                                                # category 5: false positives on a grid; rank 101 covers the second ground truth
            k5 += 1                                          # this detection's rank within the category
            if k5 == 101:
                dets.append(([560, 400, 619, 459], pool.pop(), 1))
            else:
                x, y = 50 + 44 * (k5 % 11), 10 + 38 * (k5 // 11)
                dets.append(([x, y, x + 30, y + 24], pool.pop(), 1))
    assert k5 == 102 and k9 == 12
    second = [_ann(c[2], [100, 100, 20, 20]), _ann(c[0], [300, 200, 50, 40])]
    dets2 = [([100, 100, 119, 109.5], pool.pop(), 3), ([300, 200, 349, 239], pool.pop(), 1), ([204, 306, 260, 361], pool.pop(), 2),
             (dv._random_box(g), pool.pop(), 3), (dv._random_box(g), pool.pop(), 1)]
    samples = [dict(image_id=1, annotations=anns), dict(image_id=2, annotations=second)]
    trap = [([560, 400, 619, 459], 1), ([100, 100, 119, 119], 3)]
    return dict(categories=CAP_CATEGORIES, samples=samples, det=dv._pack([dets, dets2], 120, trap))


def _wide(seed):
    g = detgen._rng("cocoeval:wide", seed)
    c = [k["id"] for k in WIDE_CATEGORIES]
    anns, dets = [], []
    pool = list(dv._score_pool(g, 260))
    for i in range(70):
        x, y = 8 + 62 * (i % 10), 6 + 66 * (i // 10)
        w, h = round(float(g.uniform(22, 52)), 1), round(float(g.uniform(22, 56)), 1)
        anns.append(_ann(c[0], [x, y, w, h], iscrowd=1 if i in (64, 66, 69) else 0))
    for i in range(200):
        if i < 130:
            a = anns[int(g.integers(70)) if i >= 24 else (64, 66, 69)[i % 3]]          # the crowd regions are met several times
            dets.append((dv._jitter(g, a["bbox"], float(g.uniform(0.01, 0.25))), pool.pop(), 1))
        else:
            dets.append((dv._random_box(g), pool.pop(), 1))
    anns += [_ann(c[1], [500, 400, 100, 60]), _ann(c[1], [20, 420, 70, 50])]
    dets += [(dv._jitter(g, anns[70]["bbox"], 0.05), pool.pop(), 2), (dv._jitter(g, anns[71]["bbox"], 0.2), pool.pop(), 2), (dv._random_box(g), pool.pop(), 2)]
    second = [_ann(c[0], [100 + 120 * i, 100, 80, 90]) for i in range(4)]
    dets2 = [(dv._jitter(g, second[i % 4]["bbox"], float(g.uniform(0.02, 0.3))), pool.pop(), 1) for i in range(30)]
    samples = [dict(image_id=1, annotations=anns), dict(image_id=2, annotations=second)]
    trap = [(dv._jitter(g, anns[3]["bbox"], 0.0), 1), (dv._jitter(g, second[0]["bbox"], 0.0), 1)]
    return dict(categories=WIDE_CATEGORIES, samples=samples, det=dv._pack([dets, dets2], 208, trap))


def _identity():
    k = dv.case_inputs("apeval_small")
    samples = [dict(image_id=s["image_id"], annotations=[dict(bbox=a["bbox"], area=a["area"], category_id=a["category_id"], iscrowd=0)
                                                         for a in s["annotations"]]) for s in k["samples"]]
    assert int(k["det"].count.max()) < 300
    return dict(categories=[dict(id=c["id"]) for c in k["categories"]], samples=samples, det=k["det"])


def lvis_side():
    """coco_lvis_identity as the LVIS protocol takes it -> (categories with frequencies, samples with the federated lists)"""
    k = dv.case_inputs("apeval_small")
    ids = [c["id"] for c in k["categories"]]
    samples = [dict(image_id=s["image_id"], neg_category_ids=list(ids), not_exhaustive_category_ids=[],
                    annotations=[dict(bbox=a["bbox"], area=a["area"], category_id=a["category_id"]) for a in s["annotations"]])
               for s in k["samples"]]
    return k["categories"], samples


# ---- the restatement: one number at a time ----------------------------------------------------------------------------------------------
def det_xywh(box, plus_one):
    """BoxList.convert("xywh"): the differences and the + TO_REMOVE in fp32, then double"""
    b = [np.float32(v) for v in box]
    w, h = np.float32(b[2] - b[0]), np.float32(b[3] - b[1])
    if plus_one:
        w, h = np.float32(w + np.float32(1)), np.float32(h + np.float32(1))
    return [np.float64(b[0]), np.float64(b[1]), np.float64(w), np.float64(h)]


def iou_coco(d, g, crowd):
    """maskUtils.iou on two (x, y, w, h) boxes of np.float64"""
    zero = np.float64(0)
    iw = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    ih = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    inter = zero if iw <= 0 or ih <= 0 else iw * ih
    da = d[2] * d[3]
    return inter / da if crowd else inter / (da + g[2] * g[3] - inter)


def _check(case, k, plus_ones):
    det, exact = k["det"], {(b, d, j): v for b, d, j, v in EXACT[case]}
    met = set()
    for plus_one in plus_ones:
        for b, s in enumerate(k["samples"]):
            for d in range(int(det.count[b])):
                cid = k["categories"][int(det.labels[b, d]) - 1]["id"]
                box = det_xywh(det.boxes[b, d], plus_one)
                assert box[2] > 0 and box[3] > 0
                for j, a in enumerate(s["annotations"]):
                    if a["category_id"] != cid:
                        continue
                    v = iou_coco(box, [np.float64(x) for x in a["bbox"]], bool(a["iscrowd"]))
                    if (b, d, j) in exact:
                        assert v == exact[b, d, j] and (IOU_THRS == v).any(), (case, b, d, j, v)
                        met.add((b, d, j))
                    else:
                        assert np.abs(IOU_THRS - v).min() >= MARGIN, (case, plus_one, b, d, j, v)
    assert met == set(exact), case
    for ci in range(len(k["categories"])):
        scores = [float(det.scores[b, d]) for b in range(len(k["samples"])) for d in range(int(det.count[b])) if int(det.labels[b, d]) == ci + 1]
        assert len(scores) == len(set(scores)), (case, ci)


def case_inputs(case):
    """-> dict(categories, samples (as pack_coco_targets takes them), det (boxes / scores / labels / count, numpy), max_dets)"""
    if case not in _cache:
        spec = CASES[case]
        k = {"coco_small": lambda: _small(spec["seed"]), "coco_crowd": _crowd, "coco_cap": lambda: _cap(spec["seed"]),
             "coco_wide": lambda: _wide(spec["seed"]), "coco_lvis_identity": _identity}[case]()
        k.update(max_dets=spec["max_dets"])
        _check(case, k, spec["plus_one"])
        _cache[case] = k
    return _cache[case]


def restate_match(k, plus_one, iou_thrs=IOU_THRS, area_rng=AREA_RNG):
    """COCOeval.evaluateImg over every (image, category, area range) -> dict(match uint64 [B, D], ignore uint64 [B, D], rank int32 [B, D],
    valid uint8 [B, D], num_gt int64 [C, A])"""
    det, samples = k["det"], k["samples"]
    ids = [c["id"] for c in k["categories"]]
    B, D = det.labels.shape
    nT, nA = len(iou_thrs), len(area_rng)
    cap = k["max_dets"][-1]
    match, ignore = np.zeros((B, D), np.uint64), np.zeros((B, D), np.uint64)
    rank, valid = np.full((B, D), -1, np.int32), np.zeros((B, D), np.uint8)
    num_gt = np.zeros((len(ids), nA), np.int64)
    for b, s in enumerate(samples):
        n = min(int(det.count[b]), D)
        for ci, cid in enumerate(ids):
            gts = [dict(a, _ignore=a["iscrowd"]) for a in s["annotations"] if a["category_id"] == cid]      # 'ignore' is overwritten
            dts = sorted([d for d in range(n) if int(det.labels[b, d]) == ci + 1], key=lambda d: -float(det.scores[b, d]))
            for r, d in enumerate(dts):
                rank[b, d] = r
            dts = dts[:cap]
            for d in dts:
                valid[b, d] = 1
            boxes = {d: det_xywh(det.boxes[b, d], plus_one) for d in dts}
            for a in range(nA):
                lo, hi = np.float64(area_rng[a][0]), np.float64(area_rng[a][1])
                ig = [bool(g["_ignore"] or np.float64(g["area"]) < lo or np.float64(g["area"]) > hi) for g in gts]
                order = [j for j in range(len(gts)) if not ig[j]] + [j for j in range(len(gts)) if ig[j]]
                sgt = [gts[j] for j in order]
                sig = [ig[j] for j in order]
                num_gt[ci, a] += sum(1 for x in sig if not x)
                ious = {d: [iou_coco(boxes[d], [np.float64(v) for v in g["bbox"]], bool(g["iscrowd"])) for g in sgt] for d in dts}
                for t in range(nT):
                    bit = np.uint64(1) << np.uint64(a * nT + t)
                    gtm = [False] * len(sgt)
                    for d in dts:
                        iou = min(np.float64(iou_thrs[t]), np.float64(1 - 1e-10))
                        m = -1
                        for gind, g in enumerate(sgt):
                            if gtm[gind] and not g["iscrowd"]:
                                continue
                            if m > -1 and not sig[m] and sig[gind]:
                                break
                            if not ious[d][gind] >= iou:
                                continue
                            iou = ious[d][gind]
                            m = gind
                        area = boxes[d][2] * boxes[d][3]
                        if m == -1:
                            if area < lo or area > hi:
                                ignore[b, d] |= bit
                            continue
                        gtm[m] = True
                        match[b, d] |= bit
                        if sig[m]:
                            ignore[b, d] |= bit
    return dict(match=match, ignore=ignore, rank=rank, valid=valid, num_gt=num_gt)


def restate_accumulate(k, r, rec_thrs=REC_THRS, nT=T):
    """COCOeval.accumulate -> (precision [T, R, C, A, M], recall [T, C, A, M])"""
    det = k["det"]
    B, D = det.labels.shape
    C, nA = r["num_gt"].shape
    R, M = len(rec_thrs), len(k["max_dets"])
    precision, recall = -np.ones((nT, R, C, nA, M)), -np.ones((nT, C, nA, M))
    eps = np.float64(2.0) ** -52
    for c in range(C):
        for mi, m in enumerate(k["max_dets"]):
            rows = [(b, d) for b in range(B) for d in range(D) if r["valid"][b, d] and int(det.labels[b, d]) == c + 1 and r["rank"][b, d] < m]
            rows = sorted(rows, key=lambda x: -float(det.scores[x]))      # (sorted is stable: equal scores in arrival order)
            for a in range(nA):
                if r["num_gt"][c, a] == 0:
                    continue
                ng = np.float64(r["num_gt"][c, a])
                for t in range(nT):
                    sh = np.uint64(a * nT + t)
                    tp = fp = 0
                    rc, pr = [], []
                    for x in rows:
                        hit, ig = bool((r["match"][x] >> sh) & np.uint64(1)), bool((r["ignore"][x] >> sh) & np.uint64(1))
                        tp += int(hit and not ig)
                        fp += int(not hit and not ig)
                        rc.append(np.float64(tp) / ng)
                        pr.append(np.float64(tp) / (np.float64(fp) + np.float64(tp) + eps))
                    for i in range(len(pr) - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    recall[t, c, a, mi] = rc[-1] if rc else 0.0
                    i = 0
                    for ri in range(R):
                        while i < len(rc) and rc[i] < rec_thrs[ri]:
                            i += 1
                        precision[t, ri, c, a, mi] = pr[i] if i < len(rc) else 0.0
    return precision, recall


def restate_results(k, precision, recall, iou_thrs=IOU_THRS):
    """COCOeval.summarize for boxes; AR{m} for every m of the case's ladder"""
    def mean(values):
        values = np.asarray(values, np.float64).reshape(-1)
        values = values[values > -1]
        return -1 if len(values) == 0 else np.mean(values)
    last = len(k["max_dets"]) - 1
    res = {"AP": mean(precision[:, :, :, 0, last])}
    for key, thr in (("AP50", 0.5), ("AP75", 0.75)):
        res[key] = mean(precision[[t for t in range(len(iou_thrs)) if iou_thrs[t] == thr]][:, :, :, 0, last])
    for key, a in (("APs", 1), ("APm", 2), ("APl", 3)):
        res[key] = mean(precision[:, :, :, a, last])
    for mi, m in enumerate(k["max_dets"]):
        res[f"AR{m}"] = mean(recall[:, :, 0, mi])
    for key, a in (("ARs", 1), ("ARm", 2), ("ARl", 3)):
        res[key] = mean(recall[:, :, a, last])
    return res


def restate(case, plus_one):
    """-> dict(match, ignore, rank, valid, num_gt, precision, recall, results), once per (case, plus_one)"""
    key = ("restate", case, plus_one)
    if key not in _cache:
        k = case_inputs(case)
        r = restate_match(k, plus_one)
        r["precision"], r["recall"] = restate_accumulate(k, r)
        r["results"] = restate_results(k, r["precision"], r["recall"])
        _cache[key] = r
    return _cache[key]


def tensors(k, torch, sl=slice(None), device="cpu"):
    d = k["det"]
    return types.SimpleNamespace(boxes=torch.from_numpy(d.boxes[sl]).to(device), scores=torch.from_numpy(d.scores[sl]).to(device),
                                 labels=torch.from_numpy(d.labels[sl]).to(device), count=torch.from_numpy(d.count[sl]).to(device))
