"""Generate tests/golden/msdet_*.npz by executing the REFERENCE's multi-scale test code on the CPU (runs where the reference tree is present):

    python tools/gen_multiscale_golden.py

Executed by path behind stub parents, unmodified: structures/bounding_box.py (BoxList.transpose, resize, __getitem__),
structures/boxlist_ops.py (cat_boxlist) and data/datasets/evaluation/box_aug.py (remove_boxes, merge_result_from_multi_scales, boxlist_nms,
bbox_vote).  Stand-ins: `maskrcnn_benchmark.config.cfg` (a namespace holding the case's TEST node), the parents of the imports box_aug.py
does not use here (data.transforms, structures.image_list), and torch.Tensor.cuda patched to the identity for bbox_vote's last two lines.
The ONE stand-in that carries arithmetic is `layers.nms`, a compiled op in the reference: `greedy_nms` below is a greedy loop stating
csrc/cuda/nms.cu:15-23's rule (fp32, +1 widths, suppress iff IoU > thresh, by descending score).

Inputs by name from tests/multiscale_cases.py (the fixtures hold outputs only).  For every view case: each slot's box after the reference's
un-flip, range filter and resize, and whether it lived; for every case and both modes ("none", "vote"): the reference's merged boxes,
scores and labels per image.  Asserted, and recorded in the fixture:
  * no pair of one class and image has an fp64 IoU within 1e-4 of TH, except the listed exact-threshold pairs, which equal it in fp32;
  * no two candidates of one class and image share a score;
  * no survivors tie at the top-N cut;
  * no range-filtered area lies within 1 of a range bound, except the listed exact-bound boxes.
If a seed fails a condition, change the seed, never the condition.

vote_tol (stored in every vote fixture) = 4 x the largest |fp32 reference - fp64 recomputation of the same clusters| over ALL cases,
floored at 2 ulp of the largest coordinate.  The margin is 4 because a kernel's lane-tree summation and numpy's summation are both
within n * eps of the fp64 value but of each other only by their sum.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import shim                                      # noqa: E402
import multiscale_cases as mc                                # noqa: E402

MB = os.path.join(shim.REF, "fine_grained", "maskrcnn_benchmark")
OUT = os.path.join(ROOT, "tests", "golden")
IOU_MARGIN = 1e-4


def greedy_nms(boxes, scores, thresh):
    """layers.nms (csrc/cuda/nms.cu): indices kept, by descending score; fp32 devIoU, suppress iff > thresh"""
    b = boxes.detach().float().numpy()
    order = np.argsort(-scores.detach().float().numpy(), kind="stable")
    one, th = np.float32(1), np.float32(thresh)
    gone, keep = np.zeros(len(order), bool), []
    for n, i in enumerate(order):
        if gone[n]:
            continue
        keep.append(int(i))
        for m in range(n + 1, len(order)):
            j = order[m]
            w = max(min(b[i, 2], b[j, 2]) - max(b[i, 0], b[j, 0]) + one, np.float32(0))
            h = max(min(b[i, 3], b[j, 3]) - max(b[i, 1], b[j, 1]) + one, np.float32(0))
            inter = w * h
            sa = (b[i, 2] - b[i, 0] + one) * (b[i, 3] - b[i, 1] + one)
            sb = (b[j, 2] - b[j, 0] + one) * (b[j, 3] - b[j, 1] + one)
            if inter / (sa + sb - inter) > th:
                gone[m] = True
    return torch.tensor(keep, dtype=torch.int64)


def load_reference():
    def pkg(name, **names):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in names.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m
    mb = "maskrcnn_benchmark"
    cfg = types.SimpleNamespace(TEST=None)
    for n in (mb, mb + ".structures", mb + ".data.datasets", mb + ".data.datasets.evaluation"):
        pkg(n)
    pkg(mb + ".config", cfg=cfg)
    pkg(mb + ".data", transforms=pkg(mb + ".data.transforms"))
    pkg(mb + ".structures.image_list", to_image_list=None)
    pkg(mb + ".layers", nms=greedy_nms, ml_nms=None, soft_nms=None)
    bb = shim._load("bounding_box", os.path.join(MB, "structures", "bounding_box.py"), mb + ".structures")
    shim._load("boxlist_ops", os.path.join(MB, "structures", "boxlist_ops.py"), mb + ".structures")
    aug = shim._load("box_aug", os.path.join(MB, "data", "datasets", "evaluation", "box_aug.py"), mb + ".data.datasets.evaluation")
    torch.Tensor.cuda = lambda self, *a, **k: self           # bbox_vote ends in .float().cuda()
    return types.SimpleNamespace(BoxList=bb.BoxList, aug=aug, cfg=cfg)


def set_test(ref, classes_select, num_classes, mode, top_n):
    ref.cfg.TEST = types.SimpleNamespace(SELECT_CLASSES=list(classes_select), NUM_CLASSES=int(num_classes), TH=mc.TH,
                                         SPECIAL_NMS=mode, PRE_NMS_TOP_N=int(top_n))


# ---- the asserted conditions ---------------------------------------------------------------------------------------------------------------
def check_candidates(name, cands, classes, exact_pairs):
    """-> (smallest |IoU - TH| outside the exact pairs, smallest score gap inside a class).  cands: per image the slot lists."""
    margin, gap = np.inf, np.inf
    exact = {frozenset((a, b)) for a, b in exact_pairs}
    for b, slots in enumerate(cands):
        live = [c for c in slots if c is not None and c["label"] in classes]
        for label in sorted({c["label"] for c in live}):
            seg = [c for c in live if c["label"] == label]
            s = np.array([c["score"] for c in seg], np.float32)
            assert len(set(s.tolist())) == len(seg), f"{name} image {b} class {label}: two candidates share a score"
            if len(seg) > 1:
                gap = min(gap, float(np.diff(np.sort(s.astype(np.float64))).min()))
            bx = np.array([c["box"] for c in seg], np.float64)
            w = (np.minimum(bx[:, None, 2], bx[None, :, 2]) - np.maximum(bx[:, None, 0], bx[None, :, 0]) + 1).clip(min=0)
            h = (np.minimum(bx[:, None, 3], bx[None, :, 3]) - np.maximum(bx[:, None, 1], bx[None, :, 1]) + 1).clip(min=0)
            area = (bx[:, 2] - bx[:, 0] + 1) * (bx[:, 3] - bx[:, 1] + 1)
            o = w * h / (area[:, None] + area[None, :] - w * h)
            d = np.abs(o - mc.TH)
            np.fill_diagonal(d, np.inf)
            for i, j in zip(*np.nonzero(d < IOU_MARGIN)):
                pair = frozenset((seg[i]["box"], seg[j]["box"]))
                assert pair in exact, f"{name} image {b} class {label}: IoU {o[i, j]!r} within {IOU_MARGIN} of TH: change the seed"
                b32 = bx.astype(np.float32)
                assert np.float32(mc.iou(b32[i], b32[j])) == np.float32(mc.TH) and o[i, j] == mc.TH, "the exact pair is not exact"
                d[i, j] = np.inf
            margin = min(margin, float(d.min()) if len(seg) > 1 else np.inf)
    return margin, gap


def check_areas(name, case):
    """-> smallest distance of a filtered area to a range bound outside the listed exact-bound boxes (scaled frame, after the un-flip)"""
    dist = np.inf
    for view in case["views"]:
        if view["range"] is None:
            continue
        for b in range(len(case["originals"])):
            for box, score in zip(view["boxes"][b], view["scores"][b]):
                if score < 0:
                    continue
                area = (box[2] - box[0] + 1.0) * (box[3] - box[1] + 1.0)
                d = min(abs(area - view["range"][0] ** 2), abs(area - view["range"][1] ** 2))
                if box in case["exact_areas"]:
                    assert d == 0, f"{name}: {box} is listed as sitting on a bound"
                else:
                    assert d >= 1, f"{name}: area {area} within 1 of a bound of {view['range']}: change the seed"
                    dist = min(dist, d)
    return dist


# ---- the reference's own code on the cases -------------------------------------------------------------------------------------------------
def reference_collect(ref, case):
    """-> (per image the reference's concatenated BoxList, t_boxes fp32 [B, T, 4], t_live bool [B, T]): box_aug.im_detect_bbox_aug's
    bookkeeping with the model's outputs replaced by the case's candidates"""
    B = len(case["originals"])
    T = sum(len(v["boxes"][0]) for v in case["views"])
    t_boxes, t_live = np.zeros((B, T, 4), np.float32), np.zeros((B, T), bool)
    per_image = [[] for _ in range(B)]
    off = 0
    for view in case["views"]:
        lists, slots = [], []
        for b, (H, W) in enumerate(case["originals"]):
            oh, ow = view["sizes"][b]
            sc = np.array(view["scores"][b], np.float32)
            idx = np.nonzero(sc >= 0)[0]
            bl = ref.BoxList(torch.tensor([view["boxes"][b][i] for i in idx], dtype=torch.float32).view(-1, 4), (ow, oh), mode="xyxy")
            bl.add_field("scores", torch.from_numpy(sc[idx]))
            bl.add_field("labels", torch.tensor([view["labels"][b][i] for i in idx], dtype=torch.int64))
            bl.add_field("slot", torch.from_numpy(idx + off))
            lists.append(bl.transpose(0) if view["flip"] else bl)
        if view["range"] is not None:
            lists = ref.aug.remove_boxes(lists, *view["range"])
        for b, (H, W) in enumerate(case["originals"]):
            r = lists[b].resize((W, H))
            assert r.bbox.dtype == torch.float32
            s = r.get_field("slot").numpy()
            t_boxes[b, s], t_live[b, s] = r.bbox.numpy(), True
            per_image[b].append(r)
        off += len(view["boxes"][0])
    merged = []
    for b, lists in enumerate(per_image):
        bl = ref.BoxList(torch.cat([x.bbox for x in lists]), lists[0].size, lists[0].mode)
        bl.add_field("scores", torch.cat([x.get_field("scores") for x in lists]))
        bl.add_field("labels", torch.cat([x.get_field("labels") for x in lists]))
        merged.append(bl)
    return merged, t_boxes, t_live


def boxlists_of(ref, cands):
    """the common-frame candidates of a merge case as the reference's concatenated BoxLists"""
    out = []
    for slots in cands:
        live = [c for c in slots if c is not None]
        bl = ref.BoxList(torch.tensor([c["box"] for c in live], dtype=torch.float32).view(-1, 4), (4096, 4096), mode="xyxy")
        bl.add_field("scores", torch.tensor([c["score"] for c in live], dtype=torch.float32))
        bl.add_field("labels", torch.tensor([c["label"] for c in live], dtype=torch.int64))
        out.append(bl)
    return out


def reference_merge(ref, boxlists):
    """-> per image (boxes fp32 [n, 4], scores fp32 [n], labels int64 [n]) sorted by descending score, then label"""
    out = []
    for r in ref.aug.merge_result_from_multi_scales(boxlists):
        bx, sc, lb = r.bbox.float().numpy(), r.get_field("scores").float().numpy(), r.get_field("labels").numpy()
        order = np.lexsort((lb, -sc.astype(np.float64)))
        out.append((bx[order], sc[order], lb[order]))
    return out


def save(name, mode, got, want, extra):
    """got: the reference's per-image results; want: the restatement's (uncut survivor count checked against the reference's)"""
    B, R = len(got), max(max(len(g[1]) for g in got), 1)
    bx, sc, lb, cnt = np.zeros((B, R, 4), np.float32), np.full((B, R), -1, np.float32), np.zeros((B, R), np.int32), np.zeros(B, np.int32)
    err, top = 0.0, 0.0
    for b, (gb, gs, gl) in enumerate(got):
        n = len(gs)
        bx[b, :n], sc[b, :n], lb[b, :n], cnt[b] = gb, gs, gl, n
        kept = want[b]
        assert n == len(kept), f"{name} {mode} image {b}: the reference keeps {n}, the restatement {len(kept)}"
        if n:
            assert [c["label"] for c in kept] == gl.tolist() and [np.float32(c["score"]) for c in kept] == gs.tolist(), f"{name} {mode} image {b}"
            ref64 = np.array([c["box"] for c in kept], np.float64)
            err = max(err, float(np.abs(gb.astype(np.float64) - ref64).max()))
            top = max(top, float(np.abs(gb).max()))
    return dict(path=os.path.join(OUT, mc.golden_name(name, mode) + ".npz"), data=dict(boxes=bx, scores=sc, labels=lb, count=cnt, **extra)), err, top


def cut_is_tie_free(name, mode, uncut, top_n):
    """no survivors tie at the top-N cut: the N-th and (N + 1)-th scores differ"""
    for b, kept in enumerate(uncut):
        if len(kept) > top_n:
            assert kept[top_n - 1]["score"] != kept[top_n]["score"], f"{name} {mode} image {b}: survivors tie at the cut: change the seed"


def main():
    torch.set_num_threads(8)
    ref = load_reference()
    files, errs, tops = [], [0.0], [0.0]
    for name in mc.VIEW_CASES:
        case = mc.view_case(name)
        cfg = case["cfg"]
        cands = mc.collect_ref(case)
        margin, gap = check_candidates(name, cands, case["classes"], case["exact_pairs"])
        area_margin = check_areas(name, case)
        boxlists, t_boxes, t_live = reference_collect(ref, case)
        # the restatement's collect against the reference's, slot by slot and bit for bit
        mine_b, mine_s, *_ = mc.cands_to_arrays(cands)
        assert np.array_equal(mine_s >= 0, t_live) and np.array_equal(mine_b.view(np.int32), t_boxes.view(np.int32)), name
        for mode in mc.MODES:
            set_test(ref, cfg["select"], cfg["num_classes"], mode, cfg["top_n"])
            got = reference_merge(ref, boxlists)
            uncut = mc.merge_ref(cands, case["classes"], mc.TH, mode, 1 << 30)
            cut_is_tie_free(name, mode, uncut, cfg["top_n"])
            f, err, top = save(name, mode, got, [k[:cfg["top_n"]] for k in uncut],
                               dict(t_boxes=t_boxes, t_live=t_live, iou_margin=np.float64(margin), score_gap=np.float64(gap),
                                    area_margin=np.float64(area_margin)))
            files.append((f, mode)), errs.append(err if mode == "vote" else 0.0), tops.append(top)
            print(name, mode, "kept", [len(g[1]) for g in got], "iou margin", f"{margin:.3e}", "area margin", area_margin)
    for name in mc.MERGE_CASES:
        cands, classes, _ = mc.merge_case(name)
        margin, gap = check_candidates(name, cands, classes, mc.MERGE_EXACT[name])
        boxlists = boxlists_of(ref, cands)
        for mode in mc.MODES:
            uncut = mc.merge_ref(cands, classes, mc.TH, mode, 1 << 30)
            top_n = max(max(len(k) for k in uncut) // 2, 1)                      # the cut bites in the largest image
            cut_is_tie_free(name, mode, uncut, top_n)
            set_test(ref, classes, 0, mode, top_n)
            got = reference_merge(ref, boxlists)
            f, err, top = save(name, mode, got, [k[:top_n] for k in uncut],
                               dict(top_n=np.int64(top_n), iou_margin=np.float64(margin), score_gap=np.float64(gap)))
            files.append((f, mode)), errs.append(err if mode == "vote" else 0.0), tops.append(top)
            print(name, mode, "kept", [len(g[1]) for g in got], "top_n", top_n, "iou margin", f"{margin:.3e}", "vote err", f"{err:.3e}")
    floor = 2 * float(np.spacing(np.float32(max(tops))))
    vote_tol = max(4 * max(errs), floor)
    print("vote_tol", vote_tol, "(4 x", max(errs), ", floor", floor, ")")
    for f, mode in files:
        if mode == "vote":
            f["data"]["vote_tol"] = np.float64(vote_tol)
        np.savez_compressed(f["path"], **f["data"])


if __name__ == "__main__":
    main()
