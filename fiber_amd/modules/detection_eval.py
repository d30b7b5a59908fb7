"""Box average precision of the fine-grained model by the LVIS protocol and by the COCO protocol, on the device.

The LVIS protocol first; the COCO protocol (CocoBoxEvaluator) is described after it by what differs.  Mirrors fine_grained/maskrcnn_benchmark/data/datasets/evaluation/lvis/lvis_eval.py: Params (:52-76), LVISResults.limit_dets_per_image
(:137-148), LVISEval._prepare / compute_iou / evaluate_img / accumulate / _summarize / summarize (:201-586), LvisEvaluator (:637-750) and
LvisEvaluatorFixedAP (:767-872).

The reference copies every prediction to the host and walks images x categories x four area ranges x ten IoU thresholds in Python.  Here
the Detections stay where they are:
  pack_detection_targets  the batch's annotations as fixed-shape tensors (DetectionTargets)
  evaluator.update        ONE launch of ops.ap_match (csrc/apeval.hip, one wave per (image, area range, threshold)): per detection slot a
                          64-bit match word, a 64-bit ignore word (bit a * T + t) and a valid byte; num_gt is added to.  No synchronisation.
  evaluator.tables        the records of all updates ranked by two stable sorts (score, then category), ONE launch of ops.ap_accumulate
  evaluator.summarize     the one device-to-host copy (the two tables), then the reference's means with numpy
On CPU tensors the same bookkeeping runs with the two launches replaced by numpy (_match_host, _accumulate_host), which the `not gpu`
tests hold against fixtures the reference's own LVISEval produced.

Why matching is per batch and truncation post hoc: the greedy rule is order-dependent only among the detections of one (image, category),
and LvisEvaluatorFixedAP's per-category top k is a prefix of that category's score order.  A record inside the prefix has every
higher-scoring detection of its image and category inside it too, so its match is the one the reference finds after truncating.  The
records are therefore matched when they arrive and cut to each category's k best at the end; the k best are counted before the federated
filter drops any, as the reference counts them.

Deviations from the reference:
  * two detections of one category with EQUAL scores are ranked in arrival order (update order, then image, then slot); the reference's
    order then depends on its sorted image ids.
  * a ground-truth box of zero or negative extent and a repeated image id are refused; the reference's 0 / 0 would match as NaN, and its
    np.unique keeps one of the repeats.
  * rec_thrs must ascend (the reference's searchsorted assumes it).

Two protocols share the records, the ordering, the accumulation kernel and the rank gather (_RecordEvaluator); make_box_evaluator picks
one by name, and evaluator.pack_targets packs a batch's annotations for it.

"lvis": BoxAPEvaluator, everything above.

"coco": CocoBoxEvaluator, the protocol of the reference's COCO fine-tuning and ODinW configs (TEST ("coco_2017_val",), EVAL_TASK
"detection": evaluation/coco/coco_eval.py:125-154 prepare_for_coco_detection, :366-386 COCOeval evaluate / accumulate / summarize,
:389-445 summarize_per_category).  PARITY UNPINNED against the pycocotools binary: pycocotools is neither in the reference tree nor
available to the tests, so the rule is implemented from its statement (include/fiber_hip.h, fiber_ap_match_coco) and no fixture of
COCOeval's own output exists.  What pins it instead: on inputs without crowd, ignore or federated lists the tables are array_equal to
BoxAPEvaluator's, which the reference's LVISEval fixtures pin; the hand-worked bits of the crowd and cap cases; the independent scalar
restatement of tests/coco_eval_cases.py.  The differences from the LVIS protocol:
  pack_coco_targets       CocoTargets: iscrowd in place of ignore (a stray "ignore" key is discarded, as COCOeval overwrites it), no
                          negative / not-exhaustive lists: every category is evaluated in every image
  evaluator.update        ONE launch of ops.ap_match_coco: a crowd ground truth divides the intersection by the DETECTION's area, can be
                          matched again and counts as ignored; only the first maxDets[-1] = 100 detections of an (image, category)
                          exist (the cap is per category, not per image); the detection's extents carry the reference's + TO_REMOVE
                          (plus_one); besides the words and the valid byte, each slot's rank within its (image, category)
  evaluator.tables        per m of maxDets (1, 10, 100) the records with rank < m and ONE launch of ops.ap_accumulate:
                          precision [T, R, C, A, M], recall [T, C, A, M]
  evaluator.summarize     AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl; per_category() the rows of the reference's CSV
Equal scores within a category rank in arrival order there too (the first deviation above): COCOeval's mergesort over its sorted image
ids may order them otherwise.

Out of scope: segmentation and keypoint IoU, evaluate_box_proposals (box_only), the JSON / TSV / CSV result writers, LvisDumper, the
dataset readers and the contiguous-id mapping (callers pass category ids), check_expected_results.

evaluate_detection runs one prompt per image; evaluate_detection_chunked a vocabulary cut into prompts (detection_prompts.py), with the
prompt-independent part of the backbone computed once per image, the image-independent part once per evaluation and the chunks of an image
merged by ops.det_merge; evaluate_detection_multiscale one prompt per image over the views of TEST.SCALES x TEST.FLIP
(box_aug.im_detect_bbox_aug: GeneralizedVLRCNN.detect_multiscale, merged by ops.det_aug_merge with plain NMS or box voting).  Out of
scope there: sharing the FPN lateral of the prompt-independent level between an image's pairs, multi-scale testing of a chunked
vocabulary, TEST.SPECIAL_NMS "soft-nms" / "soft-vote", and the result CSV writers.
"""
import numpy as np
import torch

from .. import ops

MAX_GT = 4096                                                # = ops.ap_max_gt(); the host path keeps the same bound
MAX_COCO_CATEGORIES = 4096                                   # = ops.ap_coco_max_categories(); the host path keeps the same bound
FREQUENCIES = ("r", "c", "f")
AREA_LABELS = ("all", "small", "medium", "large")


def default_params():
    """Params (:52-76): (iou_thrs [10], rec_thrs [101], area_rng [4, 2]) as numpy computes them"""
    iou_thrs = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
    rec_thrs = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
    area_rng = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)
    return iou_thrs, rec_thrs, area_rng


class DetectionTargets:
    """Ground truth of one batch: gt fp64 [B, G, 4] (xywh, original frame), area fp64 [B, G] (the annotation's own field), category int32
    [B, G] (index into the sorted category ids), ignore uint8 [B, G], gt_count int32 [B], neg_mask / nel_mask int64 [B, ceil(C / 64)]
    (the bits of a uint64: bit c of word c // 64 = category c is in the image's negative / not-exhaustive list); image_ids (host list of
    B) and category_ids (host list of C) travel along."""

    def __init__(self, gt, area, category, ignore, gt_count, neg_mask, nel_mask, image_ids, category_ids):
        self.gt, self.area, self.category, self.ignore, self.gt_count = gt, area, category, ignore, gt_count
        self.neg_mask, self.nel_mask = neg_mask, nel_mask
        self.image_ids, self.category_ids = list(image_ids), list(category_ids)

    def to(self, device):
        return DetectionTargets(*(t.to(device) for t in (self.gt, self.area, self.category, self.ignore, self.gt_count, self.neg_mask,
                                                         self.nel_mask)), self.image_ids, self.category_ids)


def _category_ids(categories):
    ids = [c["id"] for c in categories]
    if not ids or ids != sorted(set(ids)):
        raise ValueError("categories: a non-empty list of {'id', 'frequency'} in ascending id order without repeats")
    for c in categories:
        if c["frequency"] not in FREQUENCIES:
            raise ValueError(f"categories: frequency {c['frequency']!r} of category {c['id']} is none of {FREQUENCIES}")
    return ids


def _mask_words(ids, index, words, what, image_id):
    out = np.zeros(words, dtype=np.uint64)
    for i in ids:
        if i not in index:
            raise ValueError(f"pack_detection_targets: image {image_id}: {what} names category {i}, which is not in categories")
        out[index[i] >> 6] |= np.uint64(1) << np.uint64(index[i] & 63)
    return out.view(np.int64)


def pack_detection_targets(samples, categories, num_boxes=None):
    """samples: one dict per image with "image_id", "annotations" (the dataset's own: "bbox" xywh, "area", "category_id", optional
    "ignore"), "neg_category_ids" and "not_exhaustive_category_ids".  categories: [{"id", "frequency"}] in ascending id order.
    num_boxes fixes G (default: the batch's maximum, at least 1).  -> DetectionTargets on the host."""
    ids = _category_ids(categories)
    index = {c: i for i, c in enumerate(ids)}
    B, W = len(samples), (len(ids) + 63) // 64
    most = max([len(s["annotations"]) for s in samples] + [0])
    G = max(most, 1)
    if num_boxes is not None:
        if num_boxes < most:
            raise ValueError(f"pack_detection_targets: an image has {most} annotations, more than num_boxes = {num_boxes}")
        G = max(int(num_boxes), 1)
    if G > MAX_GT:
        raise ValueError(f"pack_detection_targets: {G} ground-truth boxes per image exceed the matching kernel's capacity of {MAX_GT}")
    gt, area = np.zeros((B, G, 4), np.float64), np.zeros((B, G), np.float64)
    cat, ign, cnt = np.zeros((B, G), np.int32), np.zeros((B, G), np.uint8), np.zeros((B,), np.int32)
    neg, nel = np.zeros((B, W), np.int64), np.zeros((B, W), np.int64)
    for b, s in enumerate(samples):
        for g, ann in enumerate(s["annotations"]):
            box = np.asarray(ann["bbox"], dtype=np.float64).reshape(4)
            if not np.isfinite(box).all() or not np.isfinite(ann["area"]):
                raise ValueError(f"pack_detection_targets: image {s['image_id']} annotation {g}: non-finite box or area")
            if box[2] <= 0 or box[3] <= 0:
                raise ValueError(f"pack_detection_targets: image {s['image_id']} annotation {g}: ground-truth box of no extent")
            if ann["category_id"] not in index:
                raise ValueError(f"pack_detection_targets: image {s['image_id']} annotation {g}: category {ann['category_id']} not in categories")
            gt[b, g], area[b, g], cat[b, g], ign[b, g] = box, ann["area"], index[ann["category_id"]], 1 if ann.get("ignore", 0) else 0
        cnt[b] = len(s["annotations"])
        neg[b] = _mask_words(s.get("neg_category_ids", ()), index, W, "neg_category_ids", s["image_id"])
        nel[b] = _mask_words(s.get("not_exhaustive_category_ids", ()), index, W, "not_exhaustive_category_ids", s["image_id"])
    return DetectionTargets(*(torch.from_numpy(x) for x in (gt, area, cat, ign, cnt, neg, nel)), [s["image_id"] for s in samples], ids)


def _match_host(boxes, labels, count, t, iou_thrs, area_rng, num_gt, max_dets):
    """ops.ap_match on CPU tensors, in numpy: one fp64 rounding per operation in the order the kernel's header states.
    num_gt is accumulated in place.  -> (match, ignore, valid)"""
    bx = boxes.detach().float().numpy()
    lab, cnt = labels.numpy(), count.numpy()
    gt, garea, gcat, gign, gcnt = t.gt.numpy(), t.area.numpy(), t.category.numpy(), t.ignore.numpy(), t.gt_count.numpy()
    neg, nel = t.neg_mask.numpy().view(np.uint64), t.nel_mask.numpy().view(np.uint64)
    thrs, rng, ngt = iou_thrs.numpy(), area_rng.numpy(), num_gt.numpy()
    B, D = lab.shape
    C, A = ngt.shape
    T = len(thrs)
    match, ignore, valid = np.zeros((B, D), np.uint64), np.zeros((B, D), np.uint64), np.zeros((B, D), np.uint8)
    w = (bx[:, :, 2] - bx[:, :, 0]).astype(np.float64)       # fp32 differences, then double
    h = (bx[:, :, 3] - bx[:, :, 1]).astype(np.float64)
    x, y = bx[:, :, 0].astype(np.float64), bx[:, :, 1].astype(np.float64)
    darea = w * h
    floor = np.minimum(thrs, 1 - 1e-10)

    def listed(words, b, c):
        return bool((words[b, c >> 6] >> np.uint64(c & 63)) & np.uint64(1))
    for b in range(B):
        n = min(max(int(cnt[b]), 0), D)
        if max_dets >= 0:
            n = min(n, max_dets)
        m = min(max(int(gcnt[b]), 0), gt.shape[1])
        cats, g, ga, gi = gcat[b, :m], gt[b, :m], garea[b, :m], gign[b, :m] != 0
        for a in range(A):
            out = gi | (ga < rng[a, 0]) | (ga > rng[a, 1])
            np.add.at(ngt[:, a], cats[~out], 1)
        for c in np.unique(lab[b, :n] - 1):
            c = int(c)
            if not 0 <= c < C:
                continue
            mine = np.nonzero(cats == c)[0]
            if len(mine) == 0 and not listed(neg, b, c):
                continue
            dets = np.nonzero(lab[b, :n] - 1 == c)[0]
            valid[b, dets] = 1
            lazy = listed(nel, b, c)
            iw = (np.minimum((x[b, dets] + w[b, dets])[:, None], g[mine, 0] + g[mine, 2]) - np.maximum(x[b, dets][:, None], g[mine, 0])).clip(min=0)
            ih = (np.minimum((y[b, dets] + h[b, dets])[:, None], g[mine, 1] + g[mine, 3]) - np.maximum(y[b, dets][:, None], g[mine, 1])).clip(min=0)
            inter = iw * ih
            iou = inter / (darea[b, dets][:, None] + g[mine, 2] * g[mine, 3] - inter)
            for a in range(A):
                lo, hi = rng[a]
                out = gi[mine] | (ga[mine] < lo) | (ga[mine] > hi)
                small = (darea[b, dets] < lo) | (darea[b, dets] > hi) | lazy
                for ti in range(T):
                    bit = np.uint64(1) << np.uint64(a * T + ti)
                    free = np.ones(len(mine), bool)
                    for k, d in enumerate(dets):
                        ok = free & (iou[k] >= floor[ti])
                        pick = ok & ~out if (ok & ~out).any() else ok
                        if pick.any():
                            best = iou[k][pick].max()
                            j = np.nonzero(pick & (iou[k] == best))[0][-1]      # the later one on an exact tie
                            free[j] = False
                            match[b, d] |= bit
                            if out[j]:
                                ignore[b, d] |= bit
                        elif small[k]:
                            ignore[b, d] |= bit
    return torch.from_numpy(match.view(np.int64)), torch.from_numpy(ignore.view(np.int64)), torch.from_numpy(valid)


class CocoTargets:
    """Ground truth of one batch for the COCO protocol: gt fp64 [B, G, 4] (xywh, original frame), area fp64 [B, G] (the annotation's own
    field), category int32 [B, G] (index into the sorted category ids), crowd uint8 [B, G] (iscrowd), gt_count int32 [B]; image_ids
    (host list of B) and category_ids (host list of C) travel along.  There are no federated lists."""

    def __init__(self, gt, area, category, crowd, gt_count, image_ids, category_ids):
        self.gt, self.area, self.category, self.crowd, self.gt_count = gt, area, category, crowd, gt_count
        self.image_ids, self.category_ids = list(image_ids), list(category_ids)

    def to(self, device):
        return CocoTargets(*(t.to(device) for t in (self.gt, self.area, self.category, self.crowd, self.gt_count)), self.image_ids,
                           self.category_ids)


def _coco_category_ids(categories):
    ids = [c["id"] for c in categories]
    if not ids or ids != sorted(set(ids)):
        raise ValueError("categories: a non-empty list of {'id'} in ascending id order without repeats")
    if len(ids) > MAX_COCO_CATEGORIES:
        raise ValueError(f"categories: {len(ids)} exceed the matching kernel's {MAX_COCO_CATEGORIES} rank counters")
    return ids


def pack_coco_targets(samples, categories, num_boxes=None):
    """samples: one dict per image with "image_id" and "annotations" (the dataset's own: "bbox" xywh, "area", "category_id", "iscrowd";
    a stray "ignore" is accepted and discarded, as COCOeval overwrites it with iscrowd).  categories: [{"id"}] in ascending id order.
    num_boxes fixes G (default: the batch's maximum, at least 1).  The refusals are pack_detection_targets'.  -> CocoTargets on the host."""
    ids = _coco_category_ids(categories)
    index = {c: i for i, c in enumerate(ids)}
    B = len(samples)
    most = max([len(s["annotations"]) for s in samples] + [0])
    G = max(most, 1)
    if num_boxes is not None:
        if num_boxes < most:
            raise ValueError(f"pack_coco_targets: an image has {most} annotations, more than num_boxes = {num_boxes}")
        G = max(int(num_boxes), 1)
    if G > MAX_GT:
        raise ValueError(f"pack_coco_targets: {G} ground-truth boxes per image exceed the matching kernel's capacity of {MAX_GT}")
    seen = set()
    gt, area = np.zeros((B, G, 4), np.float64), np.zeros((B, G), np.float64)
    cat, crowd, cnt = np.zeros((B, G), np.int32), np.zeros((B, G), np.uint8), np.zeros((B,), np.int32)
    for b, s in enumerate(samples):
        if s["image_id"] in seen:
            raise ValueError(f"pack_coco_targets: image {s['image_id']} appears more than once")
        seen.add(s["image_id"])
        for g, ann in enumerate(s["annotations"]):
            box = np.asarray(ann["bbox"], dtype=np.float64).reshape(4)
            if not np.isfinite(box).all() or not np.isfinite(ann["area"]):
                raise ValueError(f"pack_coco_targets: image {s['image_id']} annotation {g}: non-finite box or area")
            if box[2] <= 0 or box[3] <= 0:
                raise ValueError(f"pack_coco_targets: image {s['image_id']} annotation {g}: ground-truth box of no extent")
            if ann["category_id"] not in index:
                raise ValueError(f"pack_coco_targets: image {s['image_id']} annotation {g}: category {ann['category_id']} not in categories")
            gt[b, g], area[b, g], cat[b, g], crowd[b, g] = box, ann["area"], index[ann["category_id"]], 1 if ann.get("iscrowd", 0) else 0
        cnt[b] = len(s["annotations"])
    return CocoTargets(*(torch.from_numpy(x) for x in (gt, area, cat, crowd, cnt)), [s["image_id"] for s in samples], ids)


def _match_coco_host(boxes, labels, count, t, iou_thrs, area_rng, num_gt, cap, plus_one):
    """ops.ap_match_coco on CPU tensors, in numpy: one fp64 rounding per operation in the order the kernel's header states.
    num_gt is accumulated in place.  -> (match, ignore, rank, valid)"""
    bx = boxes.detach().float().numpy()
    lab, cnt = labels.numpy(), count.numpy()
    gt, garea, gcat, gcrowd, gcnt = t.gt.numpy(), t.area.numpy(), t.category.numpy(), t.crowd.numpy(), t.gt_count.numpy()
    thrs, rng, ngt = iou_thrs.numpy(), area_rng.numpy(), num_gt.numpy()
    B, D = lab.shape
    C, A = ngt.shape
    T = len(thrs)
    match, ignore = np.zeros((B, D), np.uint64), np.zeros((B, D), np.uint64)
    rank, valid = np.full((B, D), -1, np.int32), np.zeros((B, D), np.uint8)
    w32, h32 = bx[:, :, 2] - bx[:, :, 0], bx[:, :, 3] - bx[:, :, 1]           # fp32 differences
    if plus_one:
        w32, h32 = w32 + np.float32(1), h32 + np.float32(1)                  # + TO_REMOVE, still fp32
    w, h = w32.astype(np.float64), h32.astype(np.float64)
    x, y = bx[:, :, 0].astype(np.float64), bx[:, :, 1].astype(np.float64)
    darea = w * h
    floor = np.minimum(thrs, 1 - 1e-10)
    for b in range(B):
        n = min(max(int(cnt[b]), 0), D)
        m = min(max(int(gcnt[b]), 0), gt.shape[1])
        cats, g, ga, crowd = gcat[b, :m], gt[b, :m], garea[b, :m], gcrowd[b, :m] != 0
        known = (cats >= 0) & (cats < C)
        for a in range(A):
            out = crowd | (ga < rng[a, 0]) | (ga > rng[a, 1])
            np.add.at(ngt[:, a], cats[known & ~out], 1)
        for c in np.unique(lab[b, :n] - 1):
            c = int(c)
            if not 0 <= c < C:
                continue
            slots = np.nonzero(lab[b, :n] - 1 == c)[0]
            rank[b, slots] = np.arange(len(slots), dtype=np.int32)
            dets = slots[:cap]                               # only the first maxDets[-1] of an (image, category) exist
            valid[b, dets] = 1
            mine = np.nonzero(cats == c)[0]
            iw = np.minimum((x[b, dets] + w[b, dets])[:, None], g[mine, 0] + g[mine, 2]) - np.maximum(x[b, dets][:, None], g[mine, 0])
            ih = np.minimum((y[b, dets] + h[b, dets])[:, None], g[mine, 1] + g[mine, 3]) - np.maximum(y[b, dets][:, None], g[mine, 1])
            inter = np.where((iw <= 0) | (ih <= 0), 0.0, iw * ih)
            cr = crowd[mine]
            with np.errstate(divide="ignore", invalid="ignore"):             # a detection of no area: NaN, which reaches no threshold
                iou = np.where(cr[None, :], inter / darea[b, dets][:, None], inter / (darea[b, dets][:, None] + g[mine, 2] * g[mine, 3] - inter))
            for a in range(A):
                lo, hi = rng[a]
                out = cr | (ga[mine] < lo) | (ga[mine] > hi)
                small = (darea[b, dets] < lo) | (darea[b, dets] > hi)
                for ti in range(T):
                    bit = np.uint64(1) << np.uint64(a * T + ti)
                    free = np.ones(len(mine), bool)
                    for k, d in enumerate(dets):
                        ok = (free | cr) & (iou[k] >= floor[ti])             # a crowd region can be matched again
                        pick = ok & ~out if (ok & ~out).any() else ok
                        if pick.any():
                            best = iou[k][pick].max()
                            j = np.nonzero(pick & (iou[k] == best))[0][-1]      # the later one on an exact tie
                            free[j] = bool(cr[j])
                            match[b, d] |= bit
                            if out[j]:
                                ignore[b, d] |= bit
                        elif small[k]:
                            ignore[b, d] |= bit
    return (torch.from_numpy(match.view(np.int64)), torch.from_numpy(ignore.view(np.int64)), torch.from_numpy(rank),
            torch.from_numpy(valid))


def _accumulate_host(match, ignore, seg_ptr, num_gt, rec_thrs, T):
    """ops.ap_accumulate on CPU tensors, in numpy"""
    m, ig, seg, ngt, thr = match.numpy().view(np.uint64), ignore.numpy().view(np.uint64), seg_ptr.numpy(), num_gt.numpy(), rec_thrs.numpy()
    C, A = ngt.shape
    R = len(thr)
    precision, recall = np.full((T, R, C, A), -1.0), np.full((T, C, A), -1.0)
    eps = np.spacing(np.float64(1))
    for c in range(C):
        rows = slice(int(seg[c]), int(seg[c + 1]))
        for a in range(A):
            if ngt[c, a] == 0:
                continue
            for t in range(T):
                sh = np.uint64(a * T + t)
                hit, skip = ((m[rows] >> sh) & np.uint64(1)).astype(bool), ((ig[rows] >> sh) & np.uint64(1)).astype(bool)
                tp = np.cumsum(hit & ~skip).astype(np.float64)
                fp = np.cumsum(~hit & ~skip).astype(np.float64)
                rc = tp / np.float64(ngt[c, a])
                pr = tp / (fp + tp + eps)
                pr = np.maximum.accumulate(pr[::-1])[::-1]
                at = np.searchsorted(rc, thr, side="left")
                if len(pr) == 0:                             # ground truth and no record: precision 0, recall 0
                    precision[t, :, c, a], recall[t, c, a] = 0.0, 0.0
                    continue
                precision[t, :, c, a] = np.where(at < len(pr), pr[np.minimum(at, len(pr) - 1)], 0.0)
                recall[t, c, a] = rc[-1]
    return torch.from_numpy(precision), torch.from_numpy(recall)


class _RecordEvaluator:
    """What the two protocols share: the thresholds, the per-update records (flat columns of dtypes COLUMNS, the first two the scores
    and the labels), num_gt, the rank gather and the ordering the accumulation takes."""
    COLUMNS = ()

    def _params(self, iou_thrs, rec_thrs, area_rng):
        d_iou, d_rec, d_area = default_params()
        self.iou_thrs = np.asarray(d_iou if iou_thrs is None else iou_thrs, dtype=np.float64).reshape(-1)
        self.rec_thrs = np.asarray(d_rec if rec_thrs is None else rec_thrs, dtype=np.float64).reshape(-1)
        self.area_rng = np.asarray(d_area if area_rng is None else area_rng, dtype=np.float64).reshape(-1, 2)
        if len(self.iou_thrs) == 0 or len(self.area_rng) == 0 or len(self.iou_thrs) * len(self.area_rng) > 64:
            raise ValueError(f"{len(self.iou_thrs)} IoU thresholds x {len(self.area_rng)} area ranges: between 1 and the 64 bits of a record's "
                             "match word")
        if (np.diff(self.rec_thrs) < 0).any():
            raise ValueError("rec_thrs must ascend")
        self.num_gt = self._iou = self._rec = self._area = None

    def reset(self):
        """Forget every update.  num_gt is zeroed in place."""
        self._records = []                                   # per update: one flat tensor per entry of COLUMNS
        self.image_ids = []
        self._tables = None
        self.results = None
        if self.num_gt is not None:
            self.num_gt.zero_()

    def _state(self, device, targets):
        if list(targets.category_ids) != self.category_ids:
            raise ValueError("update: targets packed with other categories than the evaluator's")
        if self.num_gt is None:
            self.num_gt = torch.zeros((len(self.category_ids), len(self.area_rng)), dtype=torch.int64, device=device)
            self._iou, self._rec, self._area = (torch.from_numpy(x.copy()).to(device) for x in (self.iou_thrs, self.rec_thrs, self.area_rng))
        elif self.num_gt.device != device:
            raise ValueError(f"update: tensors on {device}, earlier ones on {self.num_gt.device}")

    def _begin(self, detections, targets, boxes):
        """the checks every update starts with -> (boxes, labels int32, count int32)"""
        boxes = detections.boxes if boxes is None else boxes
        dev = boxes.device
        B = boxes.shape[0]
        if len(targets.image_ids) != B or targets.gt.shape[0] != B or targets.gt.device != dev:
            raise ValueError(f"update: targets of {len(targets.image_ids)} samples on {targets.gt.device} for {B} images on {dev}")
        if targets.gt.shape[1] > MAX_GT:
            raise ValueError(f"update: {targets.gt.shape[1]} ground-truth boxes per image exceed the capacity of {MAX_GT}")
        self._state(dev, targets)
        return boxes, detections.labels.to(torch.int32), detections.count.to(torch.int32)

    def _gathered(self):
        dev = self.num_gt.device
        if not self._records:
            return tuple(torch.zeros(0, dtype=dtype, device=dev) for dtype in self.COLUMNS)
        return tuple(torch.cat(col) for col in zip(*self._records))

    def synchronize(self):
        """Data-parallel evaluation: every rank ends up with the records of all (all_gather, padded to the largest count) and the
        summed num_gt (all_reduce).  The identity in a single-process run."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return
        if self.num_gt is None:
            raise RuntimeError("synchronize: no update on this rank yet (the device of the tables is unknown)")
        world, dev = dist.get_world_size(), self.num_gt.device
        cols = self._gathered()
        n = torch.tensor([cols[0].numel()], dtype=torch.int64, device=dev)
        counts = [torch.zeros_like(n) for _ in range(world)]
        dist.all_gather(counts, n)
        counts = [int(c) for c in counts]
        most = max(counts)
        merged = []
        for col in cols:
            sent = col.to(torch.uint8) if col.dtype == torch.bool else col
            pad = torch.zeros(most, dtype=sent.dtype, device=dev)
            pad[:sent.numel()] = sent
            parts = [torch.zeros_like(pad) for _ in range(world)]
            dist.all_gather(parts, pad)
            merged.append(torch.cat([p[:k] for p, k in zip(parts, counts)]).to(col.dtype))
        ids = [None] * world
        dist.all_gather_object(ids, self.image_ids)
        dist.all_reduce(self.num_gt)
        self._records = [tuple(merged)]
        self.image_ids = [i for part in ids for i in part]
        self._tables = None

    def _ordered(self, scores, cat):
        """the permutation by category, then by descending score, stable in arrival order; the sorted categories"""
        by_score = torch.sort(scores, descending=True, stable=True).indices
        cats, by_cat = torch.sort(cat[by_score], stable=True)
        return by_score[by_cat], cats

    def _accumulated(self, scores, cat, keep, match, ignore):
        """the kept records in the order of _ordered and ONE launch of ops.ap_accumulate (on CPU tensors _accumulate_host)"""
        C, dev = len(self.category_ids), self.num_gt.device
        kept = torch.where(keep, cat, torch.full_like(cat, C))                # dropped records sort behind the last category
        order, cats = self._ordered(scores, kept)
        seg_ptr = torch.searchsorted(cats, torch.arange(C + 1, device=dev))
        args = (match[order].contiguous(), ignore[order].contiguous(), seg_ptr, self.num_gt, self._rec, len(self.iou_thrs))
        return ops.ap_accumulate(*args) if dev.type == "cuda" else _accumulate_host(*args)

    def _mean(self, s):
        s = s[s > -1]
        return -1 if len(s) == 0 else np.mean(s)

    def _host_tables(self):
        """refuses a repeated image id; the one device-to-host copy -> (precision, recall) as numpy"""
        seen = set()
        for i in self.image_ids:
            if i in seen:
                raise ValueError(f"summarize: image {i} was given to update more than once")
            seen.add(i)
        precision, recall = self.tables()
        flat = torch.cat((precision.reshape(-1), recall.reshape(-1))).cpu().numpy()       # the one device-to-host copy
        return flat[:precision.numel()].reshape(precision.shape), flat[precision.numel():].reshape(recall.shape)


class BoxAPEvaluator(_RecordEvaluator):
    """LvisEvaluator + LVISEval for boxes; with fixed_ap_topk = k, LvisEvaluatorFixedAP: no cap per image, every category keeps its k
    best records over the whole set."""
    COLUMNS = (torch.float32, torch.int32, torch.int64, torch.int64, torch.uint8, torch.bool)       # scores, labels, match, ignore, valid, ranked
    pack_targets = staticmethod(pack_detection_targets)

    def __init__(self, categories, max_dets=300, fixed_ap_topk=None, iou_thrs=None, rec_thrs=None, area_rng=None):
        self.category_ids = _category_ids(categories)
        self.freq_groups = [[i for i, c in enumerate(categories) if c["frequency"] == f] for f in FREQUENCIES]
        self._params(iou_thrs, rec_thrs, area_rng)
        if fixed_ap_topk is not None and int(fixed_ap_topk) <= 0:
            raise ValueError(f"fixed_ap_topk {fixed_ap_topk}: a positive number of records per category")
        self.fixed_ap_topk = None if fixed_ap_topk is None else int(fixed_ap_topk)
        self.max_dets = -1 if self.fixed_ap_topk is not None else int(max_dets)
        self.reset()

    @property
    def image_cap(self):
        """the most detections an image may keep (LVISResults.limit_dets_per_image), None for no cut"""
        return self.max_dets if self.max_dets >= 0 else None

    def update(self, detections, targets, boxes=None):
        """detections: Detections (scores, labels and count are read; boxes too unless `boxes` fp32 [B, D, 4] gives them in the ORIGINAL
        image frame, DetImageList.boxes_to_original), targets: DetectionTargets on the same device.  One launch, no synchronisation.
        -> (match int64 [B, D], ignore int64 [B, D], valid uint8 [B, D])."""
        boxes, labels, count = self._begin(detections, targets, boxes)
        dev = boxes.device
        D = boxes.shape[1]
        if boxes.is_cuda:
            match, ignore, valid = ops.ap_match(boxes, labels, count, targets.gt, targets.area, targets.category, targets.ignore,
                                                targets.gt_count, targets.neg_mask, targets.nel_mask, self._iou, self._area, self.num_gt,
                                                self.max_dets)
        else:
            match, ignore, valid = _match_host(boxes, labels, count, targets, self._iou, self._area, self.num_gt, self.max_dets)
        limit = count.clamp(0, D)
        if self.max_dets >= 0:
            limit = limit.clamp(max=self.max_dets)
        ranked = torch.arange(D, device=dev)[None, :] < limit[:, None]       # the slots that hold a detection (:137-148)
        self._records.append((detections.scores.detach().float().reshape(-1), labels.reshape(-1), match.reshape(-1), ignore.reshape(-1),
                              valid.reshape(-1), ranked.reshape(-1)))
        self.image_ids.extend(targets.image_ids)
        self._tables = None
        return match, ignore, valid

    def tables(self):
        """-> (precision fp64 [T, R, C, A], recall fp64 [T, C, A]) on the device of the updates"""
        if self._tables is not None:
            return self._tables
        if self.num_gt is None:
            raise RuntimeError("tables: no update yet")
        C, dev = len(self.category_ids), self.num_gt.device
        scores, labels, match, ignore, valid, ranked = self._gathered()
        cat = labels.long() - 1
        edges = torch.arange(C + 1, device=dev)
        keep = valid.bool() & ranked
        if self.fixed_ap_topk is not None:                   # the k best of a category, counted before the federated filter (:776-788)
            every = torch.where(ranked & (cat >= 0) & (cat < C), cat, torch.full_like(cat, C))
            order, cats = self._ordered(scores, every)
            start = torch.searchsorted(cats, edges)
            rank = torch.empty_like(order)
            rank[order] = torch.arange(order.numel(), device=dev) - start[cats]
            keep = keep & (rank < self.fixed_ap_topk)
        self._tables = self._accumulated(scores, cat, keep, match, ignore)
        return self._tables

    def summarize(self):
        """-> the reference's `results`: AP, AP50, AP75, APs, APm, APl, APr, APc, APf and, without fixed_ap_topk, AR@{max_dets},
        ARs@.., ARm@.., ARl@.. (:551-584); the mean over entries > -1, or -1 for an empty selection (:526-549).  A repeated image id
        raises ValueError.  The one place that synchronises."""
        precision, recall = self._host_tables()
        area = {name: i for i, name in enumerate(AREA_LABELS[:len(self.area_rng)])}

        def at(thr):
            return np.where(thr == self.iou_thrs)[0]
        res = {"AP": self._mean(precision[:, :, :, area["all"]]),
               "AP50": self._mean(precision[at(0.50)][:, :, :, area["all"]]),
               "AP75": self._mean(precision[at(0.75)][:, :, :, area["all"]])}
        for key, name in (("APs", "small"), ("APm", "medium"), ("APl", "large")):
            res[key] = self._mean(precision[:, :, :, area[name]]) if name in area else -1
        for key, group in zip(("APr", "APc", "APf"), self.freq_groups):
            res[key] = self._mean(precision[:, :, np.asarray(group, dtype=np.intp), area["all"]])
        if self.fixed_ap_topk is None:
            res[f"AR@{self.max_dets}"] = self._mean(recall[:, :, area["all"]])
            for name in ("small", "medium", "large"):
                res[f"AR{name[0]}@{self.max_dets}"] = self._mean(recall[:, :, area[name]]) if name in area else -1
        self.results = res
        return res


class CocoBoxEvaluator(_RecordEvaluator):
    """COCOeval for boxes (evaluate / accumulate / summarize) with the COCO API's parameters: maxDets (1, 10, 100) per (image, category),
    the crowd rule, no federated lists.  plus_one: the detection extents carry the reference's + TO_REMOVE (prepare_for_coco_detection);
    False for callers that hold true xywh extents."""
    COLUMNS = (torch.float32, torch.int32, torch.int64, torch.int64, torch.uint8, torch.int32)      # scores, labels, match, ignore, valid, rank
    METRICS = ("AP", "AP50", "AP75", "APs", "APm", "APl")    # COCOResults.METRICS["bbox"] (coco_eval.py:456-471)
    pack_targets = staticmethod(pack_coco_targets)
    image_cap = None                                         # the cap is per (image, category): nothing is cut per image

    def __init__(self, categories, max_dets=(1, 10, 100), iou_thrs=None, rec_thrs=None, area_rng=None, plus_one=True):
        self.category_ids = _coco_category_ids(categories)
        self._params(iou_thrs, rec_thrs, area_rng)
        self.max_dets = tuple(int(m) for m in max_dets)
        if not self.max_dets or self.max_dets[0] <= 0 or any(a >= b for a, b in zip(self.max_dets, self.max_dets[1:])):
            raise ValueError(f"max_dets {max_dets}: positive numbers of detections per (image, category), ascending")
        self.plus_one = bool(plus_one)
        self.reset()

    def update(self, detections, targets, boxes=None):
        """detections: Detections (scores, labels and count are read; boxes too unless `boxes` fp32 [B, D, 4] gives them in the ORIGINAL
        image frame, DetImageList.boxes_to_original), targets: CocoTargets on the same device.  One launch, no synchronisation.
        -> (match int64 [B, D], ignore int64 [B, D], rank int32 [B, D], valid uint8 [B, D])."""
        boxes, labels, count = self._begin(detections, targets, boxes)
        args = (boxes, labels, count)
        if boxes.is_cuda:
            match, ignore, rank, valid = ops.ap_match_coco(*args, targets.gt, targets.area, targets.category, targets.crowd, targets.gt_count,
                                                           self._iou, self._area, self.num_gt, self.max_dets[-1], self.plus_one)
        else:
            match, ignore, rank, valid = _match_coco_host(*args, targets, self._iou, self._area, self.num_gt, self.max_dets[-1], self.plus_one)
        self._records.append((detections.scores.detach().float().reshape(-1), labels.reshape(-1), match.reshape(-1), ignore.reshape(-1),
                              valid.reshape(-1), rank.reshape(-1)))
        self.image_ids.extend(targets.image_ids)
        self._tables = None
        return match, ignore, rank, valid

    def tables(self):
        """-> (precision fp64 [T, R, C, A, M], recall fp64 [T, C, A, M]) on the device of the updates: per m of max_dets the records
        with rank < m, ordered as BoxAPEvaluator orders its own, and one launch of ops.ap_accumulate."""
        if self._tables is not None:
            return self._tables
        if self.num_gt is None:
            raise RuntimeError("tables: no update yet")
        scores, labels, match, ignore, valid, rank = self._gathered()
        cat = labels.long() - 1
        per_m = [self._accumulated(scores, cat, valid.bool() & (rank < m), match, ignore) for m in self.max_dets]
        self._tables = torch.stack([p for p, _ in per_m], dim=-1), torch.stack([r for _, r in per_m], dim=-1)
        return self._tables

    def _empty(self):
        C, A, M = len(self.category_ids), len(self.area_rng), len(self.max_dets)
        return np.full((len(self.iou_thrs), len(self.rec_thrs), C, A, M), -1.0), np.full((len(self.iou_thrs), C, A, M), -1.0)

    def _at(self, thr):
        return np.where(thr == self.iou_thrs)[0]

    def summarize(self):
        """-> COCOeval.summarize for boxes: AP, AP50, AP75, APs, APm, APl (the reference's COCOResults.METRICS["bbox"]) at the largest
        max_dets, AR{m} over all areas for every m of max_dets (AR1, AR10, AR100), ARs, ARm, ARl at the largest; the mean over entries
        > -1, or -1 for an empty selection.  An evaluator without an update summarises to -1 everywhere.  A repeated image id raises
        ValueError.  The one place that synchronises."""
        precision, recall = self._empty() if self.num_gt is None else self._host_tables()
        area = {name: i for i, name in enumerate(AREA_LABELS[:len(self.area_rng)])}
        precision, last = precision[..., -1], recall[..., -1]
        res = {"AP": self._mean(precision[:, :, :, area["all"]]),
               "AP50": self._mean(precision[self._at(0.50)][:, :, :, area["all"]]),
               "AP75": self._mean(precision[self._at(0.75)][:, :, :, area["all"]])}
        for key, name in (("APs", "small"), ("APm", "medium"), ("APl", "large")):
            res[key] = self._mean(precision[:, :, :, area[name]]) if name in area else -1
        for i, m in enumerate(self.max_dets):
            res[f"AR{m}"] = self._mean(recall[:, :, area["all"], i])
        for key, name in (("ARs", "small"), ("ARm", "medium"), ("ARl", "large")):
            res[key] = self._mean(last[:, :, area[name]]) if name in area else -1
        self.results = res
        return res

    def per_category(self):
        """-> {"category_ids": [C], "AP", "AP50", "APs", "APm", "APl": fp64 [C]}: the rows summarize_per_category writes
        (coco_eval.py:389-445), each the PLAIN mean of the category's precision entries at the largest max_dets, -1 entries included, as
        the reference takes it.  (The reference leaves a row out when no entry of the metric exceeds -1; here it is all -1.)"""
        precision = (self._empty() if self.num_gt is None else self._host_tables())[0][..., -1]
        area = {name: i for i, name in enumerate(AREA_LABELS[:len(self.area_rng)])}
        C = len(self.category_ids)

        def row(sel, name):
            if name not in area or sel.shape[0] == 0:
                return np.full(C, -1.0)
            return np.array([np.mean(sel[:, :, c, area[name]]) for c in range(C)])
        out = {"category_ids": list(self.category_ids), "AP": row(precision, "all"), "AP50": row(precision[self._at(0.50)], "all")}
        for key, name in (("APs", "small"), ("APm", "medium"), ("APl", "large")):
            out[key] = row(precision, name)
        return out


def make_box_evaluator(protocol, categories, **kw):
    """protocol "lvis" -> BoxAPEvaluator, "coco" -> CocoBoxEvaluator; kw goes to the constructor.  Either one serves evaluate_detection,
    evaluate_detection_chunked and evaluate_detection_multiscale; evaluator.pack_targets packs the batch's "targets" for it."""
    kinds = {"lvis": BoxAPEvaluator, "coco": CocoBoxEvaluator}
    if protocol not in kinds:
        raise ValueError(f"make_box_evaluator: protocol {protocol!r} is none of {tuple(kinds)}")
    return kinds[protocol](categories, **kw)


def evaluate_detection(model, batches, evaluator):
    """The detection loop of engine/inference.py, batched, as evaluate_grounding runs the grounding one.  batches yields dicts with
    "images" (a DetImageList), "tokenizer_input", "positive_maps" and "targets" (what evaluator.pack_targets returns: DetectionTargets
    for a BoxAPEvaluator, CocoTargets for a CocoBoxEvaluator).  -> evaluator.summarize().  Nothing synchronises before summarize."""
    model.eval()
    with torch.no_grad():
        for batch in batches:
            images = batch["images"]
            detections = model(images, tokenizer_input=batch["tokenizer_input"], positive_map=batch["positive_maps"])
            boxes = images.boxes_to_original(detections)
            evaluator.update(detections, batch["targets"].to(boxes.device), boxes=boxes)
    return evaluator.summarize()


def evaluate_detection_multiscale(model, batches, evaluator, test_cfg=None):
    """The detection loop with test-time augmentation (TEST.USE_MULTISCALE: engine/inference.py:47-48 and :492-504, im_detect_bbox_aug).
    batches yields dicts as evaluate_detection takes them, except that "images" is the list of raw uint8 [H, W, 3] device tensors:
    GeneralizedVLRCNN.detect_multiscale resizes and flips them per view itself and returns boxes in each image's original frame.
    test_cfg: the TEST node (default model.cfg.TEST).  -> evaluator.summarize().  Nothing synchronises before summarize."""
    model.eval()
    with torch.no_grad():
        for batch in batches:
            detections = model.detect_multiscale(batch["images"], tokenizer_input=batch["tokenizer_input"], positive_map=batch["positive_maps"],
                                                 test_cfg=test_cfg)
            evaluator.update(detections, batch["targets"].to(detections.boxes.device), boxes=detections.boxes)
    return evaluator.summarize()


def evaluate_detection_chunked(model, batches, evaluator, prompts, prompts_per_pass=None):
    """The detection loop over a vocabulary too large for one prompt (TEST.CHUNKED_EVALUATION: LVIS, 1203 categories as 31 prompts of
    40).  prompts: detection_prompts.build_detection_prompts over the evaluator's categories; their text prefix is encoded once
    (GeneralizedVLRCNN.encode_prompts), every batch then goes through detect_chunked, which merges an image's chunks on the device and cuts
    to the evaluator's max_dets as LVISResults.limit_dets_per_image does (:137-148; no cut with fixed_ap_topk, :790-795).  batches yields
    dicts with "images" (a DetImageList) and "targets" (DetectionTargets).  -> evaluator.summarize().  Nothing synchronises before
    summarize."""
    if list(prompts.category_ids) != list(evaluator.category_ids):
        raise ValueError("evaluate_detection_chunked: the prompts were built over other categories than the evaluator's")
    model.eval()
    max_dets = evaluator.image_cap                           # COCO caps per (image, category) while matching: no cut per image
    with torch.no_grad():
        state = model.encode_prompts(prompts)
        for batch in batches:
            images = batch["images"]
            detections = model.detect_chunked(images, state, prompts_per_pass, max_dets=max_dets)
            boxes = images.boxes_to_original(detections)
            evaluator.update(detections, batch["targets"].to(boxes.device), boxes=boxes)
    return evaluator.summarize()
