"""Cases of multi-scale test-time augmentation (ops.det_aug_collect / ops.det_aug_merge, GeneralizedVLRCNN.detect_multiscale) and an
INDEPENDENT host restatement of box_aug.py's collect + merge in plain Python loops over lists; nothing here imports fiber_amd.ops.

Two kinds of case, both named and seeded:
  VIEW_CASES   per-view candidates in the views' resized frames (integer coordinates) with the view geometry: un-flip, range filter,
               resize, then the merge.  tools/gen_multiscale_golden.py runs the reference's own BoxList / box_aug code on them.
  MERGE_CASES  candidates already in the common frame (integer coordinates), built to corner the merge kernel: the reference's
               merge_result_from_multi_scales runs on them too.

The restatement decides in double on the fp32 box values: the fixtures' margin conditions (no IoU within 1e-4 of the threshold but the
listed exact pairs, which are 0.5 in any precision; no area within 1 of a range bound but the listed exact ones) make every decision the
one fp32 arithmetic takes.  The un-flip, the area and the resize are evaluated in fp32 (numpy.float32 scalars), bit for bit the
reference's.  Voted boxes are computed in double: they are the fp64 recomputation the fixtures' vote_tol is measured against.
"""
import numpy as np

F = np.float32
TH = 0.5
MODES = ("none", "vote")
WG = 256                                                     # the merge kernel's workgroup size
MUTATIONS = ("nms_ge", "vote_gt", "no_plus_one", "range_nonstrict", "range_after_resize", "keep_other_labels")


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def iou(a, b, plus_one=True):
    one = 1.0 if plus_one else 0.0
    w = max(min(a[2], b[2]) - max(a[0], b[0]) + one, 0.0)
    h = max(min(a[3], b[3]) - max(a[1], b[1]) + one, 0.0)
    inter = w * h
    union = (a[2] - a[0] + one) * (a[3] - a[1] + one) + (b[2] - b[0] + one) * (b[3] - b[1] + one) - inter
    return inter / union if union > 0 else 0.0


def _in_range(x1, y1, x2, y2, keep_range, strict):
    area = (x2 - x1 + F(1)) * (y2 - y1 + F(1))               # fp32
    lo, hi = F(float(keep_range[0] * keep_range[0])), F(float(keep_range[1] * keep_range[1]))
    return (lo < area < hi) if strict else (lo <= area <= hi)


def collect_ref(case, mutate=None):
    """-> per image the T slots in view order: None (dead) or dict(box (4 python floats holding fp32 values), score, label, source,
    view, slot).  Labels are NOT filtered here: merge_ref drops the ones outside the class list."""
    out = []
    for b, (H, W) in enumerate(case["originals"]):
        slots = []
        for v, view in enumerate(case["views"]):
            oh, ow = view["sizes"][b]
            rw, rh = float(W) / float(ow), float(H) / float(oh)
            for box, score, label, source in zip(view["boxes"][b], view["scores"][b], view["labels"][b], view["source"][b]):
                slot = len(slots)
                if score < 0:
                    slots.append(None)
                    continue
                x1, y1, x2, y2 = (F(c) for c in box)
                if view["flip"]:
                    x1, x2 = F(ow) - x2 - F(1), F(ow) - x1 - F(1)
                keep = True
                if view["range"] is not None and mutate != "range_after_resize":
                    keep = _in_range(x1, y1, x2, y2, view["range"], mutate != "range_nonstrict")
                if rw == rh:
                    x1, y1, x2, y2 = x1 * F(rw), y1 * F(rw), x2 * F(rw), y2 * F(rw)
                else:
                    x1, y1, x2, y2 = x1 * F(rw), y1 * F(rh), x2 * F(rw), y2 * F(rh)
                if view["range"] is not None and mutate == "range_after_resize":
                    keep = _in_range(x1, y1, x2, y2, view["range"], True)
                slots.append(dict(box=(float(x1), float(y1), float(x2), float(y2)), score=float(F(score)), label=int(label),
                                  source=int(source), view=v, slot=slot) if keep else None)
        out.append(slots)
    return out


def merge_ref(cands, classes, thresh, mode, top_n, mutate=None):
    """cands: per image a list of slots (None or dict as collect_ref gives them) -> per image the survivors, score descending, then the
    smaller label, then the earlier slot, cut to top_n: dicts with box (python floats; voted boxes in double), score, label, source, view"""
    th = float(F(thresh))
    plus_one = mutate != "no_plus_one"
    out = []
    for slots in cands:
        live = [c for c in slots if c is not None]
        wanted = sorted(set(classes)) if mutate != "keep_other_labels" else sorted({c["label"] for c in live})
        kept = []
        for label in wanted:
            pool = sorted((c for c in live if c["label"] == label), key=lambda c: (-c["score"], c["slot"]))
            while pool:
                lead, rest, cluster = pool[0], [], [pool[0]]
                for c in pool[1:]:
                    o = iou(lead["box"], c["box"], plus_one) if thresh > 0 else -1.0
                    if mode == "vote":
                        hit = thresh > 0 and (o > th if mutate == "vote_gt" else o >= th)
                    else:
                        hit = thresh > 0 and (o >= th if mutate == "nms_ge" else o > th)
                    (cluster if hit else rest).append(c)
                won = dict(lead)
                if mode == "vote" and len(cluster) > 1:
                    total = sum(c["score"] for c in cluster)
                    won["box"] = tuple(sum(c["score"] * c["box"][i] for c in cluster) / total for i in range(4))
                    won["members"] = len(cluster)
                kept.append(won)
                pool = rest
        kept.sort(key=lambda c: (-c["score"], c["label"], c["slot"]))
        out.append(kept[:top_n])
    return out


# ---- lists <-> arrays ---------------------------------------------------------------------------------------------------------------------
def cands_to_arrays(cands, junk=False):
    """-> (boxes fp32 [B, T, 4], scores fp32, labels, source, view int32 [B, T]) as ops.det_aug_collect leaves them; junk = True fills
    the dead slots with large boxes, live-looking labels and sources under NEGATIVE scores of every size"""
    B, T = len(cands), max(len(s) for s in cands)
    bx, sc = np.zeros((B, T, 4), np.float32), np.full((B, T), -1, np.float32)
    lb, sr, vw = np.zeros((B, T), np.int32), np.full((B, T), -1, np.int32), np.full((B, T), -1, np.int32)
    for b, slots in enumerate(cands):
        assert len(slots) == T
        for i, c in enumerate(slots):
            if c is None:
                if junk:
                    bx[b, i], sc[b, i] = (0.0, 0.0, 3.0e30, 3.0e30), (-3.0e38, -1e-30, -7.5, -np.inf)[i % 4]
                    lb[b, i], sr[b, i], vw[b, i] = 1 + i % 3, 12345 + i, i % 5
                continue
            bx[b, i], sc[b, i], lb[b, i], sr[b, i], vw[b, i] = c["box"], c["score"], c["label"], c["source"], c["view"]
    return bx, sc, lb, sr, vw


def result_arrays(result, D):
    """merge_ref's lists -> (boxes fp64 [B, D, 4], scores fp32, labels, source, view int32 [B, D], count int32 [B]) with nms_ml's padding"""
    B = len(result)
    bx, sc = np.zeros((B, D, 4), np.float64), np.full((B, D), -1, np.float32)
    lb, sr, vw, cnt = np.zeros((B, D), np.int32), np.full((B, D), -1, np.int32), np.full((B, D), -1, np.int32), np.zeros(B, np.int32)
    for b, kept in enumerate(result):
        assert len(kept) <= D
        cnt[b] = len(kept)
        for i, c in enumerate(kept):
            bx[b, i], sc[b, i], lb[b, i], sr[b, i], vw[b, i] = c["box"], c["score"], c["label"], c["source"], c["view"]
    return bx, sc, lb, sr, vw, cnt


def voted_mask(result, D):
    """bool [B, D]: the survivors whose box is a vote over more than one candidate"""
    m = np.zeros((len(result), D), bool)
    for b, kept in enumerate(result):
        for i, c in enumerate(kept):
            m[b, i] = c.get("members", 1) > 1
    return m


# ---- view cases ---------------------------------------------------------------------------------------------------------------------------
# originals (H, W); per view the resized (oh, ow) of each image: image 0 keeps its size in view 0 / 1 (ratio 1) and is scaled by 3 / 2 in
# both directions in views 2 / 3 (equal ratios != 1); image 1 is 50 x 101 -> 60 x 121 there (121 = int(60 * 101 / 50): unequal ratios)
VIEW_GEOMETRY = dict(originals=[(60, 80), (50, 101)],
                     views=[dict(sizes=[(60, 80), (50, 101)], flip=False), dict(sizes=[(60, 80), (50, 101)], flip=True),
                            dict(sizes=[(90, 120), (60, 121)], flip=False), dict(sizes=[(90, 120), (60, 121)], flip=True)])
VIEW_CASES = {
    # classes: TEST.SELECT_CLASSES (label 4 lies between two allowed ones, 6 past them); ranges: TEST.RANGES per scale
    "views_select": dict(seed=3, select=(1, 2, 3, 5), num_classes=8, ranges=[(4, 1000), (8, 40)], top_n=1000),
    # classes: 1 .. NUM_CLASSES - 1; the cut bites
    "views_all": dict(seed=7, select=(), num_classes=6, ranges=[(4, 1000), (8, 40)], top_n=5),
    # len(RANGES) != len(SCALES): no range filter
    "views_norange": dict(seed=12, select=(), num_classes=8, ranges=[(4, 1000)], top_n=1000),
}
# the exact-threshold pair of image 0, view 0 (ratio 1, so it stays integral): IoU = 50 / 100 = 0.5 in every precision
EXACT_PAIR = ((0.0, 0.0, 9.0, 9.0), (0.0, 0.0, 9.0, 4.0))
EXACT_LABEL = 5
# boxes of view 2 (range (8, 40)) whose area sits ON a bound: 8 x 8 = 64 and 40 x 40 = 1600, both dropped by the strict test
EXACT_AREAS = ((20.0, 70.0, 27.0, 77.0), (60.0, 20.0, 99.0, 59.0))


def case_classes(cfg):
    return list(cfg["select"]) if len(cfg["select"]) else list(range(1, cfg["num_classes"]))


def view_case(name):
    """-> dict(originals, views [dict(sizes, flip, range, boxes [B][Nv][4], scores, labels, source)], classes, top_n, exact_pairs,
    exact_areas): objects drawn in the original frame, seen with a jitter in every view, in the view's frame and integer coordinates"""
    cfg = VIEW_CASES[name]
    g = np.random.default_rng(cfg["seed"])
    geo = VIEW_GEOMETRY
    B = len(geo["originals"])
    ranges = cfg["ranges"] if len(cfg["ranges"]) == 2 else [None, None]
    n_obj, n_pad = 9, 3
    objects = []
    for (H, W) in geo["originals"]:
        objs = []
        for _ in range(n_obj):
            w, h = int(g.integers(6, 30)), int(g.integers(6, 26))
            x, y = int(g.integers(15, W - w - 1)), int(g.integers(15, H - h - 1))
            objs.append((x, y, x + w, y + h, int(g.integers(1, 8))))
        objects.append(objs)
    total = len(geo["views"]) * (n_obj + n_pad + 4)
    views = []
    for v, gv in enumerate(geo["views"]):
        boxes, scores, labels, source = [], [], [], []
        for b, (H, W) in enumerate(geo["originals"]):
            oh, ow = gv["sizes"][b]
            pool = (np.linspace(0.06, 0.97, total)[v::len(geo["views"])] + 0.001 * b).astype(np.float32).tolist()    # distinct per image
            g.shuffle(pool)
            bb, ss, ll, rr = [], [], [], []
            for (x1, y1, x2, y2, lab) in objects[b]:
                j = g.integers(-2, 3, 4)
                sx, sy = ow / W, oh / H
                q = [min(max(round((x1 + j[0]) * sx), 0), ow - 2), min(max(round((y1 + j[1]) * sy), 0), oh - 2)]
                q += [min(max(round((x2 + j[2]) * sx), q[0] + 1), ow - 1), min(max(round((y2 + j[3]) * sy), q[1] + 1), oh - 1)]
                if gv["flip"]:                                # the view saw the mirrored image
                    q[0], q[2] = ow - 1 - q[2], ow - 1 - q[0]
                bb.append(tuple(float(c) for c in q)), ss.append(pool.pop()), ll.append(lab), rr.append(int(g.integers(0, 1 << 20)))
            extra = []
            if v == 0 and b == 0:
                extra = [(EXACT_PAIR[0], EXACT_LABEL), (EXACT_PAIR[1], EXACT_LABEL)]
            if v == 2 and b == 0:
                extra = [(EXACT_AREAS[0], 1), (EXACT_AREAS[1], 2)]
            for box, lab in extra:
                bb.append(box), ss.append(pool.pop()), ll.append(lab), rr.append(int(g.integers(0, 1 << 20)))
            while len(bb) < n_obj + n_pad + 2:                # padding as the decode kernel leaves it
                bb.append((0.0, 0.0, 0.0, 0.0)), ss.append(-1.0), ll.append(0), rr.append(-1)
            order = g.permutation(len(bb))                    # padding anywhere, not only at the end
            boxes.append([bb[i] for i in order]), scores.append([ss[i] for i in order])
            labels.append([ll[i] for i in order]), source.append([rr[i] for i in order])
        views.append(dict(sizes=gv["sizes"], flip=gv["flip"], range=ranges[v // 2], boxes=boxes, scores=scores, labels=labels, source=source))
    return dict(originals=geo["originals"], views=views, classes=case_classes(cfg), top_n=cfg["top_n"], cfg=cfg,
                exact_pairs=[EXACT_PAIR], exact_areas=list(EXACT_AREAS) if ranges[1] is not None else [])


# ---- merge cases --------------------------------------------------------------------------------------------------------------------------
def _cand(box, score, label, slot, view=0):
    return dict(box=tuple(float(c) for c in box), score=float(F(score)), label=int(label), source=1000 + slot, view=int(view), slot=slot)


def _spread(n, label, first_score, x0=0, step=40):
    """n boxes of one class that do not touch each other: every one survives"""
    return [((x0 + step * i, 0, x0 + step * i + 20, 20), first_score - 1e-4 * i, label) for i in range(n)]


def _stack(n, label, first_score, x0=0, y0=100):
    """n boxes of one class, all within IoU >= 0.8 of the first: one cluster, one survivor"""
    return [((x0, y0, x0 + 60 + (i % 3), y0 + 60 + (i % 2)), first_score - 1e-4 * i, label) for i in range(n)]


def _image(groups, dead_every=0, shuffle_seed=None):
    """groups: lists of (box, score, label) -> the slots of one image (dead slots interleaved, order shuffled)"""
    items = [it for grp in groups for it in grp]
    if shuffle_seed is not None:
        items = [items[i] for i in np.random.default_rng(shuffle_seed).permutation(len(items))]
    slots = []
    for box, score, label in items:
        if dead_every and len(slots) % dead_every == 0:
            slots.append(None)
        slots.append(_cand(box, score, label, len(slots), view=len(slots) % 4))
    return slots


def _pad(images):
    T = max(len(s) for s in images)
    return [s + [None] * (T - len(s)) for s in images]


def _layout_case():
    """B = 3 with different layouts: segments of length 0 (class 2 of image 0; class 6 everywhere), 1, 2 and 3; a segment of WG + 3 and
    one of 2 WG that survive whole, and a stack of WG + 5 that collapses into one cluster; label 4 (outside the table) between allowed
    ones; the chain; the exact-threshold pair; image 2 has no live candidate."""
    chain = [((0, 200, 99, 299), 0.90, 5), ((30, 200, 129, 299), 0.80, 5), ((60, 200, 159, 299), 0.70, 5)]     # IoU(A,B) = IoU(B,C) = 0.538, IoU(A,C) = 0.25
    pair = [((300, 300, 309, 309), 0.61, 5), ((300, 300, 309, 304), 0.60, 5)]
    img0 = _image([_spread(1, 1, 0.5), _spread(3, 3, 0.45, x0=0, step=40), _spread(2, 4, 0.95), chain, pair,
                   [(b, s, 7) for b, s, _ in _spread(WG + 3, 7, 0.40, step=25)]], dead_every=7, shuffle_seed=1)
    img1 = _image([_spread(2, 2, 0.55), _stack(WG + 5, 3, 0.85), _spread(3, 4, 0.99), [(b, s, 8) for b, s, _ in _spread(2 * WG, 8, 0.30, step=25)],
                   _stack(4, 1, 0.20, x0=400)], dead_every=5, shuffle_seed=2)
    img2 = [None] * 9
    return _pad([img0, img1, img2])


def _mid_case(seed=21, views=24, per_view=600, classes=40):
    """T = 24 x 600 seeded integer boxes, 15 objects per class seen with a jitter of +-2 in every view.  Two sightings of an object have
    IoU >= 0.67 (sides >= 41); two objects of a class are drawn with IoU < 0.15, so their sightings stay below 0.35: no pair is near TH."""
    g = np.random.default_rng(seed)
    objs = []
    for k in range(per_view):
        lab = 1 + k % classes
        while True:
            w, h = int(g.integers(40, 200)), int(g.integers(40, 200))
            x, y = int(g.integers(2, 1000 - w)), int(g.integers(2, 800 - h))
            if all(o[4] != lab or iou((x, y, x + w, y + h), (o[0], o[1], o[0] + o[2], o[1] + o[3])) < 0.15 for o in objs):
                break
        objs.append((x, y, w, h, lab))
    T = views * per_view
    scores = (0.05 + 0.9 * (g.permutation(T) + 1) / (T + 1)).astype(np.float32)
    assert len(set(scores.tolist())) == T
    slots = []
    for v in range(views):
        for (x, y, w, h, lab) in objs:
            j = g.integers(-2, 3, 4)
            slot = len(slots)
            slots.append(_cand((x + j[0], y + j[1], x + w + j[2], y + h + j[3]), scores[slot], lab, slot, view=v))
    return [slots]


MERGE_CASES = {
    # name: (builder, classes, junk in the dead slots)
    "layout": (_layout_case, (1, 2, 3, 5, 6, 7, 8), True),
    "mid": (_mid_case, tuple(range(1, 41)), False),
}
# pairs (box, box) that sit on the threshold exactly, per merge case
MERGE_EXACT = {"layout": [((300.0, 300.0, 309.0, 309.0), (300.0, 300.0, 309.0, 304.0))], "mid": []}
_BUILT = {}


def merge_case(name):
    """-> (cands per image, classes, junk)"""
    if name not in _BUILT:
        builder, classes, junk = MERGE_CASES[name]
        _BUILT[name] = (builder(), list(classes), junk)
    return _BUILT[name]


def golden_name(case, mode):
    return f"msdet_{case}_{mode}"


# ---- helpers of the tests that drive ops (handed in by the caller) ----------------------------------------------------------------------
def run_collect(ops, c, classes, device):
    """ops.det_aug_collect over the views of a view case -> the five concatenated buffers"""
    import torch
    B, T = len(c["originals"]), sum(len(v["boxes"][0]) for v in c["views"])
    out = (torch.full((B, T, 4), 77.0), torch.full((B, T), 77.0), torch.full((B, T), 77, dtype=torch.int32),
           torch.full((B, T), 77, dtype=torch.int32), torch.full((B, T), 77, dtype=torch.int32))
    out = tuple(t.to(device) for t in out)
    cls = torch.tensor(classes, dtype=torch.int32, device=device)
    off = 0
    for v, view in enumerate(c["views"]):
        args = (torch.tensor(view["boxes"], dtype=torch.float32), torch.tensor(view["scores"], dtype=torch.float32),
                torch.tensor(view["labels"], dtype=torch.int32), torch.tensor(view["source"], dtype=torch.int32))
        ops.det_aug_collect(*(t.to(device) for t in args), ops.det_aug_view_rows(c["originals"], view["sizes"], view["flip"], view["range"]),
                            cls, out, off, v)
        off += args[1].shape[1]
    return out


def filtered(cands, classes):
    """collect_ref's slots with the labels outside the class list dead, as ops.det_aug_collect leaves them"""
    return [[c if c is not None and c["label"] in classes else None for c in slots] for slots in cands]


def assert_merge_equal(got, want, voted, tol, what):
    """got: ops.det_aug_merge's six tensors; want: mc.result_arrays; boxes exact where no vote happened, within tol where one did"""
    gb, gs, gl, gr, gv, gc = (t.cpu().numpy() for t in got)
    wb, ws, wl, wr, wv, wc = want
    assert gb.dtype == np.float32 and gs.dtype == np.float32 and all(a.dtype == np.int32 for a in (gl, gr, gv, gc)), what
    assert np.array_equal(gc, wc), (what, gc, wc)
    for name, g, w in (("scores", gs, ws), ("labels", gl, wl), ("source", gr, wr), ("view", gv, wv)):
        assert np.array_equal(g, w), (what, name)
    assert np.array_equal(gb[~voted], wb[~voted].astype(np.float32)), (what, "boxes")
    if voted.any():
        err = float(np.abs(gb[voted] - wb[voted]).max())
        print(f"{what}: largest voted-box difference {err:.3e} (vote_tol {tol:.3e})")
        assert err <= tol, (what, err, tol)
