"""Cases and scalar restatement of box AP evaluation (fiber_amd/modules/detection_eval.py, csrc/apeval.hip).

`restate` is the device-independent yardstick: fiber_ap_match and fiber_ap_accumulate written out one number at a time on numpy fp64
scalars, straight from the sample lists, plus the reference's summary means.  It shares no code with the package: it groups, orders,
matches, ranks and truncates itself.  tests/test_det_eval_host.py holds it and the package's CPU path against fixtures the reference's own
LVISEval / LvisEvaluatorFixedAP produced (tools/gen_det_eval_golden.py: inputs by name from here, the fixtures hold outputs only);
tests/test_hip_det_eval.py holds the kernels against both.

Cases (the smallest shapes at which each piece can still go wrong):
  apeval_small  6 images, 5 categories over the three frequency groups (ids 3, 7, 8, 12, 20), 0-5 ground truths and 8 detections per image:
                jittered copies of ground truths plus random boxes.  Fed as one update and as two updates of 3 images.
  apeval_edge   7 categories (no rare one: APr == -1), max_dets = 4; by image:
                0  detections of category 0 and no ground truth, category 0 in the negative list (false positives)
                1  a ground truth and no detection
                2  a detection of category 2, which is in neither list (dropped); category 3 is not exhaustive and its one detection is
                   unmatched (ignored); category 1 matched
                3  category 1: an ignored ground truth packed FIRST and a non-ignored one; the detection's IoU with the ignored one is the
                   larger (0.96 against 0.82): the non-ignored one wins up to 0.80, above it the ignored one is the only one qualifying
                   and the detection is ignored.  category 4: a lone ignored ground truth and its detection (ignored at every threshold)
                4  category 0: two ground truths at bit-equal IoU 7/9 to the first detection (the later one is taken, the next detection
                   gets the earlier one at 0.86; taken the other way round it would have 0.70).  category 2: a 10 x 10 detection inside a
                   20 x 10 ground truth, IoU = 1/2 EXACTLY (every intermediate a small integer): matches at 0.5
                5  category 3: ground-truth areas of exactly 32^2 and 96^2 (inside both neighbouring ranges), a detection of area exactly
                   32^2 on the first, an unmatched detection of area exactly 32^2; count = 6 > max_dets: slots 4 and 5 are cut, and
                   slot 4 WOULD match the 96^2 ground truth.  category 5: ground truth, no detection anywhere (precision 0)
                category 6 is never seen (-1).
  apeval_wide   image 0: 70 ground truths and 200 detections of category 0 (every lane loop runs more than once), a few of category 1;
                image 1: 30 more of category 0.  Category 0 has 230 records >= 3 * fiber_ap_chunk().
  apeval_fixed  the layout of apeval_small from another seed with fixed_ap_topk = 3, fed as two updates: several categories are truncated,
                and image 0 carries the best-scoring record of a category that is in neither of its lists (truncated in, then dropped).

Conditions the generator asserts on the inputs (not measurements): every IoU of a same-category pair in an image differs from every
threshold by >= MARGIN except the pairs in EXACT, which must equal it; no two detections of one category share a score over the case.
"""
import types

import numpy as np

from oracle import detgen

MARGIN = 1e-6
FRAME = (640.0, 480.0)
IOU_THRS = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
REC_THRS = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
AREA_RNG = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)
CASES = {"apeval_small": dict(seed=0, max_dets=300, topk=None), "apeval_edge": dict(seed=0, max_dets=4, topk=None),
         "apeval_wide": dict(seed=0, max_dets=300, topk=None), "apeval_fixed": dict(seed=1, max_dets=300, topk=3)}
EXACT = {"apeval_small": [], "apeval_edge": [(4, 1, 2, 0.5)], "apeval_wide": [], "apeval_fixed": []}      # (image, slot, annotation, IoU)
SMALL_CATEGORIES = [dict(id=3, frequency="r"), dict(id=7, frequency="c"), dict(id=8, frequency="f"), dict(id=12, frequency="f"),
                    dict(id=20, frequency="c")]
EDGE_CATEGORIES = [dict(id=2, frequency="c"), dict(id=5, frequency="c"), dict(id=9, frequency="f"), dict(id=11, frequency="f"),
                   dict(id=14, frequency="c"), dict(id=17, frequency="f"), dict(id=21, frequency="c")]
WIDE_CATEGORIES = [dict(id=1, frequency="f"), dict(id=4, frequency="r")]
_cache = {}


def _ann(cat_id, xywh, area=None, ignore=None):
    a = dict(bbox=[float(v) for v in xywh], area=float(xywh[2] * xywh[3] if area is None else area), category_id=cat_id)
    if ignore is not None:
        a["ignore"] = ignore
    return a


def _pack(per_image, D, trap):
    """per_image: lists of (xyxy, score, label) -> boxes fp32 [B, D, 4], scores fp32 [B, D] (descending; -1 past count), labels int32
    [B, D], count int32 [B].  Slots past count carry `trap[b]` = (xyxy, label): a box that WOULD match, so reading past count shows."""
    B = len(per_image)
    boxes, scores = np.zeros((B, D, 4), np.float32), np.full((B, D), -1.0, np.float32)
    labels, count = np.zeros((B, D), np.int32), np.zeros((B,), np.int32)
    for b, dets in enumerate(per_image):
        dets = sorted(dets, key=lambda d: -float(np.float32(d[1])))
        assert len(dets) <= D
        for i, (box, score, label) in enumerate(dets):
            boxes[b, i], scores[b, i], labels[b, i] = np.asarray(box, np.float32), np.float32(score), label
        count[b] = len(dets)
        boxes[b, len(dets):], labels[b, len(dets):] = np.asarray(trap[b][0], np.float32), trap[b][1]
    return types.SimpleNamespace(boxes=boxes, scores=scores, labels=labels, count=count)


def _score_pool(g, n):
    """n distinct fp32 scores in (0, 1), shuffled"""
    return ((g.permutation(n) + 1.0) / (n + 1.0)).astype(np.float32)


def _random_box(g):
    x, y = g.uniform(0, FRAME[0] - 140), g.uniform(0, FRAME[1] - 140)
    w, h = g.uniform(12, 130), g.uniform(12, 130)
    return [x, y, x + w, y + h]


def _jitter(g, xywh, amount):
    x, y, w, h = xywh
    e = g.uniform(-amount, amount, 4) * np.array([w, h, w, h])
    return [x + e[0], y + e[1], x + w + e[2], y + h + e[3]]


def _small_like(name, seed, dropped):
    g = detgen._rng("apeval:" + name, seed)
    cats = SMALL_CATEGORIES
    ids = [c["id"] for c in cats]
    per_image, samples, trap = [], [], []
    pool = list(_score_pool(g, 6 * 8 + 1))
    for b, ngt in enumerate([3, 0, 5, 2, 4, 1]):
        anns = []
        for _ in range(ngt):
            x, y, w, h = g.uniform(0, 400), g.uniform(0, 300), g.uniform(14, 180), g.uniform(14, 160)
            box = [round(float(x), 2), round(float(y), 2), round(float(w), 2), round(float(h), 2)]
            anns.append(_ann(ids[int(g.integers(len(ids)))], box, area=box[2] * box[3] * float(g.uniform(0.6, 1.0)),
                             ignore=1 if g.random() < 0.15 else None))
        present = {a["category_id"] for a in anns}
        absent = [i for i in ids if i not in present]
        neg = [i for i in absent if g.random() < 0.6]
        nel = [i for i in sorted(present) if g.random() < 0.3]
        dets = []
        for k in range(8):
            if anns and k < 5:
                a = anns[int(g.integers(len(anns)))]
                label = ids.index(a["category_id"]) + 1 if g.random() < 0.85 else int(g.integers(len(ids))) + 1
                dets.append((_jitter(g, a["bbox"], [0.02, 0.06, 0.12, 0.2, 0.3][k]), pool.pop(), label))
            else:
                dets.append((_random_box(g), pool.pop(), int(g.integers(len(ids))) + 1))
        if dropped and b == 0:                               # the best record of a category that image 0 lists nowhere
            free = [i for i in ids if i not in present and i not in neg]
            if not free:
                neg = neg[1:]
                free = [i for i in ids if i not in present and i not in neg]
            dets[0] = (dets[0][0], np.float32(0.995), ids.index(free[0]) + 1)
        per_image.append(dets)
        samples.append(dict(image_id=100 + 7 * b, annotations=anns, neg_category_ids=neg, not_exhaustive_category_ids=nel))
        trap.append((_jitter(g, anns[0]["bbox"], 0.0), ids.index(anns[0]["category_id"]) + 1) if anns else ([5, 5, 50, 50], 1))
    return dict(categories=cats, samples=samples, det=_pack(per_image, 12, trap))


def _edge():
    c = [k["id"] for k in EDGE_CATEGORIES]
    im = []
    # image 0: false positives of a negative category
    im.append(dict(anns=[], neg=[c[0]], nel=[], dets=[([30, 40, 130, 120], 0.91, 1), ([300, 200, 380, 330], 0.52, 1)]))
    # image 1: ground truth, no detection
    im.append(dict(anns=[_ann(c[0], [50, 60, 120, 90])], neg=[], nel=[], dets=[]))
    # image 2: matched / dropped / unmatched of a not-exhaustive category
    im.append(dict(anns=[_ann(c[1], [40, 40, 100, 80]), _ann(c[3], [400, 300, 90, 70])], neg=[], nel=[c[3]],
                   dets=[([42.5, 41.25, 138.5, 121.75], 0.88, 2), ([200, 100, 260, 170], 0.83, 3), ([20, 300, 110, 380], 0.61, 4)]))
    # image 3: ignored ground truth first, then a non-ignored one; a lone ignored ground truth
    im.append(dict(anns=[_ann(c[1], [100, 100, 50, 50], ignore=1), _ann(c[1], [104, 102, 50, 50]), _ann(c[4], [300, 300, 60, 40], ignore=1)],
                   neg=[], nel=[], dets=[([100.5, 100.5, 150.5, 150.5], 0.79, 2), ([301, 301, 359, 341], 0.57, 5)]))
    # image 4: bit-equal IoUs and IoU = 1/2 exactly
    im.append(dict(anns=[_ann(c[0], [200, 200, 40, 40]), _ann(c[0], [200, 210, 40, 40]), _ann(c[2], [300, 300, 20, 10])], neg=[], nel=[],
                   dets=[([200, 205, 240, 245], 0.97, 1), ([200, 203, 240, 243], 0.66, 1), ([300, 300, 310, 310], 0.73, 3)]))
    # image 5: the area boundaries and the cap
    im.append(dict(anns=[_ann(c[3], [10, 10, 32, 32]), _ann(c[3], [100, 100, 96, 96]), _ann(c[5], [400, 50, 80, 120])], neg=[], nel=[],
                   dets=[([10, 10, 42, 42], 0.95, 4), ([300, 10, 332, 42], 0.85, 4), ([500, 300, 560, 380], 0.75, 4), ([250, 250, 300, 290], 0.65, 4),
                         ([101, 101, 195, 197], 0.55, 4), ([12, 300, 60, 350], 0.45, 4)]))
    samples = [dict(image_id=10 + b, annotations=x["anns"], neg_category_ids=x["neg"], not_exhaustive_category_ids=x["nel"])
               for b, x in enumerate(im)]
    trap = [([30, 40, 130, 120], 1), ([50, 60, 170, 150], 1), ([400, 300, 490, 370], 4), ([104, 102, 154, 152], 2), ([200, 200, 240, 240], 1),
            ([100, 100, 196, 196], 4)]
    return dict(categories=EDGE_CATEGORIES, samples=samples, det=_pack([x["dets"] for x in im], 8, trap))


def _wide(seed):
    g = detgen._rng("apeval:wide", seed)
    c = [k["id"] for k in WIDE_CATEGORIES]
    anns, dets = [], []
    pool = list(_score_pool(g, 260))
    for i in range(70):
        x, y = 8 + 62 * (i % 10), 6 + 66 * (i // 10)
        w, h = round(float(g.uniform(22, 52)), 1), round(float(g.uniform(22, 56)), 1)
        anns.append(_ann(c[0], [x, y, w, h], ignore=1 if i % 17 == 5 else None))
    for i in range(200):
        if i < 120:
            a = anns[int(g.integers(70))]
            dets.append((_jitter(g, a["bbox"], float(g.uniform(0.01, 0.25))), pool.pop(), 1))
        else:
            dets.append((_random_box(g), pool.pop(), 1))
    anns += [_ann(c[1], [500, 400, 100, 60]), _ann(c[1], [20, 420, 70, 50])]
    dets += [(_jitter(g, anns[70]["bbox"], 0.05), pool.pop(), 2), (_jitter(g, anns[71]["bbox"], 0.2), pool.pop(), 2), (_random_box(g), pool.pop(), 2)]
    second = [_ann(c[0], [100 + 120 * i, 100, 80, 90]) for i in range(4)]
    dets2 = [(_jitter(g, second[i % 4]["bbox"], float(g.uniform(0.02, 0.3))), pool.pop(), 1) for i in range(30)]
    samples = [dict(image_id=1, annotations=anns, neg_category_ids=[], not_exhaustive_category_ids=[]),
               dict(image_id=2, annotations=second, neg_category_ids=[c[1]], not_exhaustive_category_ids=[c[0]])]
    trap = [(_jitter(g, anns[3]["bbox"], 0.0), 1), (_jitter(g, second[0]["bbox"], 0.0), 1)]
    return dict(categories=WIDE_CATEGORIES, samples=samples, det=_pack([dets, dets2], 208, trap))


def case_inputs(case):
    """-> dict(categories, samples (as pack_detection_targets takes them), det (boxes / scores / labels / count, numpy), max_dets, topk)"""
    if case not in _cache:
        spec = CASES[case]
        k = {"apeval_small": lambda: _small_like("small", spec["seed"], False), "apeval_edge": _edge, "apeval_wide": lambda: _wide(spec["seed"]),
             "apeval_fixed": lambda: _small_like("fixed", spec["seed"], True)}[case]()
        k.update(max_dets=spec["max_dets"], topk=spec["topk"])
        _cache[case] = k
    return _cache[case]


# ---- the restatement: one number at a time ----------------------------------------------------------------------------------------------
def iou_xywh(d, g):
    """box IoU of the COCO API without crowd, on np.float64 (x, y, w, h)"""
    zero = np.float64(0)
    iw = max(min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0]), zero)
    ih = max(min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1]), zero)
    inter = iw * ih
    return inter / (d[2] * d[3] + g[2] * g[3] - inter)


def det_xywh(box):
    """convert_to_xywh: the differences in fp32, then double"""
    b = [np.float32(v) for v in box]
    return [np.float64(b[0]), np.float64(b[1]), np.float64(np.float32(b[2] - b[0])), np.float64(np.float32(b[3] - b[1]))]


def restate_match(k, iou_thrs=IOU_THRS, area_rng=AREA_RNG):
    """-> dict(match uint64 [B, D], ignore uint64 [B, D], valid uint8 [B, D], num_gt int64 [C, A])"""
    det, samples = k["det"], k["samples"]
    ids = [c["id"] for c in k["categories"]]
    B, D = det.labels.shape
    T, A = len(iou_thrs), len(area_rng)
    match, ignore, valid = np.zeros((B, D), np.uint64), np.zeros((B, D), np.uint64), np.zeros((B, D), np.uint8)
    num_gt = np.zeros((len(ids), A), np.int64)
    for b, s in enumerate(samples):
        n = int(det.count[b]) if k["max_dets"] < 0 else min(int(det.count[b]), k["max_dets"])
        for ci, cid in enumerate(ids):
            gts = [a for a in s["annotations"] if a["category_id"] == cid]
            dts = [d for d in range(n) if int(det.labels[b, d]) == ci + 1]
            for a in range(A):
                lo, hi = np.float64(area_rng[a][0]), np.float64(area_rng[a][1])
                num_gt[ci, a] += sum(1 for g in gts if not (g.get("ignore", 0) or np.float64(g["area"]) < lo or np.float64(g["area"]) > hi))
            if not dts or not (gts or cid in s["neg_category_ids"]):
                continue
            boxes = {d: det_xywh(det.boxes[b, d]) for d in dts}
            ious = {(d, j): iou_xywh(boxes[d], [np.float64(v) for v in g["bbox"]]) for d in dts for j, g in enumerate(gts)}
            for d in dts:
                valid[b, d] = 1
            for a in range(A):
                lo, hi = np.float64(area_rng[a][0]), np.float64(area_rng[a][1])
                out = [bool(g.get("ignore", 0) or np.float64(g["area"]) < lo or np.float64(g["area"]) > hi) for g in gts]
                order = [j for j in range(len(gts)) if not out[j]] + [j for j in range(len(gts)) if out[j]]
                for t in range(T):
                    bit = np.uint64(1) << np.uint64(a * T + t)
                    floor = min(np.float64(iou_thrs[t]), np.float64(1 - 1e-10))
                    taken = set()
                    for d in dts:
                        won = None
                        for want_out in (False, True):
                            best = None
                            for j in order:
                                if out[j] != want_out or j in taken or ious[d, j] < floor:
                                    continue
                                if best is None or ious[d, j] >= ious[d, best]:
                                    best = j
                            if best is not None:
                                won = best
                                break
                        area = boxes[d][2] * boxes[d][3]
                        if won is not None:
                            taken.add(won)
                            match[b, d] |= bit
                            if out[won]:
                                ignore[b, d] |= bit
                        elif area < lo or area > hi or cid in s["not_exhaustive_category_ids"]:
                            ignore[b, d] |= bit
    return dict(match=match, ignore=ignore, valid=valid, num_gt=num_gt)


def kept_records(k, valid):
    """-> per category index the kept (image, slot) records in descending score order, stable in arrival order"""
    det = k["det"]
    B, D = det.labels.shape
    C = len(k["categories"])
    out = []
    for ci in range(C):
        rows = []
        for b in range(B):
            n = int(det.count[b]) if k["max_dets"] < 0 or k["topk"] is not None else min(int(det.count[b]), k["max_dets"])
            rows += [(b, d) for d in range(n) if int(det.labels[b, d]) == ci + 1]
        rows = sorted(rows, key=lambda r: -float(det.scores[r]))          # (sorted is stable)
        if k["topk"] is not None:
            rows = rows[:k["topk"]]                          # counted before the federated filter drops any
        out.append([r for r in rows if valid[r]])
    return out


def restate_accumulate(records, match, ignore, num_gt, T, rec_thrs=REC_THRS):
    """records: per category the (image, slot) list in rank order -> (precision [T, R, C, A], recall [T, C, A])"""
    C, A = num_gt.shape
    R = len(rec_thrs)
    precision, recall = -np.ones((T, R, C, A)), -np.ones((T, C, A))
    eps = np.float64(2.0) ** -52
    for c in range(C):
        for a in range(A):
            if num_gt[c, a] == 0:
                continue
            ng = np.float64(num_gt[c, a])
            for t in range(T):
                sh = np.uint64(a * T + t)
                tp = fp = 0
                rc, pr = [], []
                for r in records[c]:
                    m, ig = bool((match[r] >> sh) & np.uint64(1)), bool((ignore[r] >> sh) & np.uint64(1))
                    tp += int(m and not ig)
                    fp += int(not m and not ig)
                    rc.append(np.float64(tp) / ng)
                    pr.append(np.float64(tp) / (np.float64(fp) + np.float64(tp) + eps))
                for i in range(len(pr) - 1, 0, -1):
                    if pr[i] > pr[i - 1]:
                        pr[i - 1] = pr[i]
                recall[t, c, a] = rc[-1] if rc else 0.0
                i = 0
                for r in range(R):                           # rec_thrs ascend: the first index with rc >= thr only moves right
                    while i < len(rc) and rc[i] < rec_thrs[r]:
                        i += 1
                    precision[t, r, c, a] = pr[i] if i < len(rc) else 0.0
    return precision, recall


def restate_results(k, precision, recall, iou_thrs=IOU_THRS):
    """lvis_eval.py:526-584 on the tables"""
    def mean(values):
        values = np.asarray(values, np.float64).reshape(-1)
        values = values[values > -1]
        return -1 if len(values) == 0 else np.mean(values)
    res = {"AP": mean(precision[:, :, :, 0])}
    for key, thr in (("AP50", 0.5), ("AP75", 0.75)):
        res[key] = mean(precision[[t for t in range(len(iou_thrs)) if iou_thrs[t] == thr]][:, :, :, 0])
    for key, a in (("APs", 1), ("APm", 2), ("APl", 3)):
        res[key] = mean(precision[:, :, :, a])
    for key, f in (("APr", "r"), ("APc", "c"), ("APf", "f")):
        group = [i for i, c in enumerate(k["categories"]) if c["frequency"] == f]
        res[key] = mean(precision[:, :, group, 0]) if group else -1
    if k["topk"] is None:
        res[f"AR@{k['max_dets']}"] = mean(recall[:, :, 0])
        for a, s in ((1, "s"), (2, "m"), (3, "l")):
            res[f"AR{s}@{k['max_dets']}"] = mean(recall[:, :, a])
    return res


def restate(case):
    """-> dict(match, ignore, valid, num_gt, records, precision, recall, results), once per case"""
    key = ("restate", case)
    if key not in _cache:
        k = case_inputs(case)
        kk = dict(k, max_dets=-1) if k["topk"] is not None else k
        r = restate_match(kk)
        r["records"] = kept_records(k, r["valid"])
        r["precision"], r["recall"] = restate_accumulate(r["records"], r["match"], r["ignore"], r["num_gt"], len(IOU_THRS))
        r["results"] = restate_results(k, r["precision"], r["recall"])
        _cache[key] = r
    return _cache[key]


def ordered_records(records):
    """the flat record order and seg_ptr the accumulate entry takes"""
    flat = [r for rows in records for r in rows]
    seg = np.cumsum([0] + [len(rows) for rows in records]).astype(np.int64)
    return flat, seg
