"""Phrase-grounding evaluation of the fine-grained model: Flickr30k Entities recall@k and RefCOCO/+/g precision@k on the device.

Mirrors fine_grained/maskrcnn_benchmark/engine/inference.py:311-327 (flickr_post_process) and :483-575 (the grounding / refexp branches of
the inference loop), data/datasets/evaluation/flickr/flickr_eval.py:210-220 (_merge_boxes), :223-258 (RecallTracker), :326-393
(Flickr30kEntitiesRecallEvaluator.evaluate), :396-443 (FlickrEvaluator) and data/datasets/refexp.py:18-88 (RefExpEvaluator).

The reference evaluates on the host, one sentence at a time: the detections are copied to the CPU, bucketed by label in Python lists, a
[0, 0, 0, 0] sentinel is appended to every bucket and numpy computes an IoU matrix per phrase.  Here the Detections stay where they are:
  pack_phrase_targets   the batch's ground truth as fixed-shape tensors: gt fp64 [B, P, G, 4], gt_count [B, P], cat_mask [B, P]
  evaluator.update      ONE launch of ops.ground_recall (csrc/geval.hip, one wave per (image, phrase)); no synchronisation
  evaluator.summarize   the one device-to-host copy: two int64 [K, 64] tables of counts
On CPU tensors both evaluators run the same arithmetic through numpy (_recall_host), which the `not gpu` tests hold against fixtures
the reference's own evaluators produced.

Deviations from the reference, each by construction of the fixed-shape form:
  * a phrase counts ONCE towards each of its categories: a phrase_type list that names one type twice counts twice in the reference.
  * a ground-truth box of zero area is refused (ValueError): the reference's 0 / 0 would poison that phrase's numpy max.
  * RefExp: a repeated image_id is skipped with a warning, as the Flickr evaluator does (the reference's dict keeps the last); an image
    without detections is a miss at every k (the reference raises on the empty zip, refexp.py:61).
  * RefExp ranks by stored position, i.e. by descending score; the reference's sorted(zip(scores, boxes)) breaks score ties by box.

Out of scope: gathering predictions across ranks (synchronize_between_processes), the csv writers (write_flickr_results,
write_refexp_results), the COCO evaluator (pycocotools; LVIS box AP is detection_eval.py) and test-time augmentation of the grounding loops (im_detect_bbox_aug
is built for detection: GeneralizedVLRCNN.detect_multiscale, detection_eval.evaluate_detection_multiscale).  Tokenisation and
the dataset readers stay with the caller, as everywhere in this package.
"""
import warnings

import numpy as np
import torch

from .. import ops

MAX_CATEGORIES = 64
MAX_K = 8
REFEXP_DATASETS = ("refcoco", "refcoco+", "refcocog")


class PhraseTargets:
    """Ground truth of one batch: gt fp64 [B, P, G, 4] (xyxy, original frame), gt_count int32 [B, P] (0 = padding row), cat_mask int64
    [B, P] (bit c = categories[c]; bit 0 = "all"); image_ids / sentence_ids (host lists of B) and categories (host list) travel along."""

    def __init__(self, gt, gt_count, cat_mask, image_ids, sentence_ids, categories):
        self.gt, self.gt_count, self.cat_mask = gt, gt_count, cat_mask
        self.image_ids, self.sentence_ids, self.categories = list(image_ids), list(sentence_ids), list(categories)

    def to(self, device):
        return PhraseTargets(self.gt.to(device), self.gt_count.to(device), self.cat_mask.to(device), self.image_ids, self.sentence_ids,
                             self.categories)


def _categories(categories):
    cats = [str(c) for c in categories]
    if "all" in cats[1:]:
        raise ValueError('categories: "all" is bit 0 (first or omitted)')
    if not cats or cats[0] != "all":
        cats = ["all"] + cats
    if len(set(cats)) != len(cats):
        raise ValueError(f"categories: repeated name in {cats}")
    if len(cats) > MAX_CATEGORIES:
        raise ValueError(f"categories: {len(cats)} with 'all' exceed the {MAX_CATEGORIES} bits of the category mask")
    return cats


def pack_phrase_targets(samples, categories, merge_boxes=False, num_phrases=None, num_boxes=None):
    """samples: one dict per image with "image_id", "sentence_id", "phrases" (a list of {"boxes": [[x1, y1, x2, y2], ...], "phrase_type":
    [names]} in label order: phrase p is label p + 1) and optionally "dataset_name" (counted as one more category: the RefExp split).
    categories: the names a phrase may count towards; "all" is bit 0 and is added when absent.  merge_boxes: each phrase's boxes are
    replaced by their enclosing box first (flickr_eval.py:210-220, FLICKR_GT_TYPE "merged").  num_phrases / num_boxes fix P / G
    (default: the batch's maxima, at least 1).  -> PhraseTargets on the host."""
    cats = _categories(categories)
    bit = {c: i for i, c in enumerate(cats)}
    B = len(samples)
    P = max([len(s["phrases"]) for s in samples] + [1])
    G = max([len(ph["boxes"]) for s in samples for ph in s["phrases"]] + [1])
    if merge_boxes:
        G = 1
    if num_phrases is not None:
        if num_phrases < P and any(len(s["phrases"]) > num_phrases for s in samples):
            raise ValueError(f"pack_phrase_targets: a sample has more than num_phrases = {num_phrases} phrases")
        P = int(num_phrases)
    if num_boxes is not None:
        if num_boxes < G and not merge_boxes and any(len(ph["boxes"]) > num_boxes for s in samples for ph in s["phrases"]):
            raise ValueError(f"pack_phrase_targets: a phrase has more than num_boxes = {num_boxes} boxes")
        G = max(int(num_boxes), 1)
    gt = np.zeros((B, P, G, 4), dtype=np.float64)
    gt_count = np.zeros((B, P), dtype=np.int32)
    cat_mask = np.zeros((B, P), dtype=np.int64)
    for b, s in enumerate(samples):
        extra = [s["dataset_name"]] if s.get("dataset_name") is not None else []
        for p, ph in enumerate(s["phrases"]):
            boxes = np.asarray(ph["boxes"], dtype=np.float64).reshape(-1, 4)
            if len(boxes) == 0:
                raise ValueError(f"pack_phrase_targets: image {s['image_id']} phrase {p} has no box (filter such phrases, flickr_eval.py:314)")
            if not np.isfinite(boxes).all():
                raise ValueError(f"pack_phrase_targets: image {s['image_id']} phrase {p}: non-finite box")
            if merge_boxes and len(boxes) > 1:
                boxes = np.array([[boxes[:, 0].min(), boxes[:, 1].min(), boxes[:, 2].max(), boxes[:, 3].max()]])
            if bool((((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])) == 0).any()):
                raise ValueError(f"pack_phrase_targets: image {s['image_id']} phrase {p}: ground-truth box of zero area")
            mask = 1
            for name in list(ph.get("phrase_type", ())) + extra:
                if str(name) not in bit:
                    raise ValueError(f"pack_phrase_targets: category {name!r} not in {cats}")
                mask |= 1 << bit[str(name)]
            gt[b, p, :len(boxes)] = boxes
            gt_count[b, p] = len(boxes)
            cat_mask[b, p] = mask if mask < (1 << 63) else mask - (1 << 64)
    return PhraseTargets(torch.from_numpy(gt), torch.from_numpy(gt_count), torch.from_numpy(cat_mask), [s["image_id"] for s in samples],
                         [s.get("sentence_id", 0) for s in samples], cats)


def _recall_host(boxes, labels, count, gt, gt_count, cat_mask, topk, positives, totals, thresh, mode):
    """ops.ground_recall on CPU tensors: the same arithmetic in numpy (fp64 IoU in mode 0, fp32 GIoU in mode 1, each operation
    rounded once in the reference's order).  positives / totals are accumulated in place.  -> (hit, best)"""
    bx = boxes.detach().float().numpy()
    lab = None if labels is None else labels.numpy()
    cnt, g, gc, cm, ks = count.numpy(), gt.numpy(), gt_count.numpy(), cat_mask.numpy(), [int(k) for k in topk.tolist()]
    B, D = bx.shape[:2]
    P, K = g.shape[1], len(ks)
    hit = np.zeros((B, P, K), dtype=np.int32)
    best = np.zeros((B, P, K), dtype=np.float64)
    pos, tot = positives.numpy(), totals.numpy()
    for b in range(B):
        n = min(max(int(cnt[b]), 0), D)
        for p in range(P):
            m = min(int(gc[b, p]), g.shape[2])
            if m <= 0:
                continue
            if mode == 0:
                d = np.concatenate([bx[b, :n][lab[b, :n] == p + 1].astype(np.float64), np.zeros((1, 4))])
                t = g[b, p, :m]
                thr = np.float64(thresh)
            else:
                d, t, thr = bx[b, :n], g[b, p, :m].astype(np.float32), np.float32(thresh)
            if len(d) == 0:
                cum = None
            else:
                area1, area2 = (d[:, 2] - d[:, 0]) * (d[:, 3] - d[:, 1]), (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])
                wh = (np.minimum(d[:, None, 2:], t[:, 2:]) - np.maximum(d[:, None, :2], t[:, :2])).clip(min=0)
                inter = wh[:, :, 0] * wh[:, :, 1]
                union = area1[:, None] + area2 - inter
                v = inter / union
                if mode == 1:
                    cwh = (np.maximum(d[:, None, 2:], t[:, 2:]) - np.minimum(d[:, None, :2], t[:, :2])).clip(min=0)
                    area = cwh[:, :, 0] * cwh[:, :, 1]
                    v = v - (area - union) / area
                cum = np.maximum.accumulate(v.max(axis=1))
            for j, k in enumerate(ks):
                if cum is None:
                    bst, h = -1.0, False
                else:
                    bst = cum[-1] if k < 0 else cum[min(k, len(cum)) - 1]
                    h = bool(bst >= thr)
                hit[b, p, j], best[b, p, j] = int(h), float(bst)
                for c in range(MAX_CATEGORIES):
                    if (int(cm[b, p]) >> c) & 1:
                        tot[j, c] += 1
                        pos[j, c] += int(h)
    return torch.from_numpy(hit), torch.from_numpy(best)


class _RecallEvaluator:
    """The bookkeeping both evaluators share: the tables of counts, the ids seen, one launch per update."""
    MODE = 0

    def __init__(self, topk, thresh):
        topk = tuple(int(k) for k in topk)
        if not 0 < len(topk) <= MAX_K or any(k == 0 or k < -1 for k in topk) or len(set(topk)) != len(topk):
            raise ValueError(f"topk {topk}: 1 to {MAX_K} distinct entries, each positive or -1 (every box)")
        self.topk, self.thresh = topk, float(thresh)
        self.categories = None
        self.evaluated_ids = set()
        self.positives = self.totals = self._topk = None
        self.results = None

    def reset(self):
        """Forget every update.  The tables are zeroed in place: a captured graph that adds to them stays valid."""
        self.categories = None
        self.evaluated_ids = set()
        self.results = None
        if self.positives is not None:
            self.positives.zero_()
            self.totals.zero_()

    def _state(self, device, categories):
        if self.categories is None:
            self.categories = list(categories)
        elif self.categories != list(categories):
            raise ValueError(f"update: targets packed with categories {categories}, earlier ones with {self.categories}")
        if self.positives is None:
            self.positives = torch.zeros((len(self.topk), MAX_CATEGORIES), dtype=torch.int64, device=device)
            self.totals = torch.zeros_like(self.positives)
            self._topk = torch.tensor(self.topk, dtype=torch.int32, device=device)
        elif self.positives.device != device:
            raise ValueError(f"update: tensors on {device}, earlier ones on {self.positives.device}")

    def update(self, boxes, detections, targets):
        """boxes fp32 [B, D, 4] in the ORIGINAL image frame (DetImageList.boxes_to_original), detections: the Detections they came from
        (labels and count are read), targets: PhraseTargets on the same device.  Launches the kernel and does not synchronise.
        -> (hit int32 [B, P, K], best fp64 [B, P, K]) on that device."""
        dev = boxes.device
        B = boxes.shape[0]
        if len(targets.image_ids) != B or targets.gt.shape[0] != B or targets.gt.device != dev:
            raise ValueError(f"update: targets of {len(targets.image_ids)} samples on {targets.gt.device} for {B} images on {dev}")
        if self.MODE == 1 and targets.gt.shape[1] != 1:
            raise ValueError(f"update: a referring expression is ONE phrase per image (targets have P = {targets.gt.shape[1]})")
        self._state(dev, targets.categories)
        keep = []
        for i, s in zip(targets.image_ids, targets.sentence_ids):
            cur = (str(i), str(s))
            if cur in self.evaluated_ids:
                warnings.warn(f"multiple predictions found for sentence {s} in image {i}: the repeat is skipped")
                keep.append(0)
            else:
                self.evaluated_ids.add(cur)
                keep.append(1)
        gt_count = targets.gt_count
        if not all(keep):
            gt_count = gt_count * torch.tensor(keep, dtype=torch.int32).to(dev)[:, None]
        labels = None if self.MODE == 1 else detections.labels
        args = (boxes, labels, detections.count, targets.gt, gt_count, targets.cat_mask, self._topk, self.positives, self.totals, self.thresh,
                self.MODE)
        if boxes.is_cuda:
            return ops.ground_recall(*args, num_categories=len(self.categories))
        return _recall_host(*args)

    def _counts(self, expected_ids):
        if expected_ids is not None:
            want = {(str(i), str(s)) for i, s in expected_ids}
            missing = sorted(want - self.evaluated_ids)
            if missing:
                raise RuntimeError("Missing predictions: " + ", ".join(f"sentence {s} in image {i}" for i, s in missing))
        if self.positives is None:
            z = np.zeros((len(self.topk), MAX_CATEGORIES), dtype=np.int64)
            return z, z
        both = torch.stack((self.positives, self.totals)).cpu().numpy()      # the one device-to-host copy
        return both[0], both[1]


class PhraseRecallEvaluator(_RecallEvaluator):
    """Flickr30kEntitiesRecallEvaluator + FlickrEvaluator.  The ground truth arrives with each update (PhraseTargets) instead of being read
    from the Flickr directory; merge_boxes is applied by pack_phrase_targets and kept here for `targets_for`."""
    MODE = 0

    def __init__(self, topk=(1, 5, 10, -1), iou_thresh=0.5, merge_boxes=False):
        super().__init__(topk, iou_thresh)
        self.merge_boxes = bool(merge_boxes)

    def targets_for(self, samples, categories, **kw):
        return pack_phrase_targets(samples, categories, merge_boxes=self.merge_boxes, **kw)

    def report(self, expected_ids=None):
        """RecallTracker.report: {k: {category: recall}} over the categories that occurred."""
        pos, tot = self._counts(expected_ids)
        cats = self.categories or ["all"]
        return {k: {c: int(pos[j, i]) / int(tot[j, i]) for i, c in enumerate(cats) if tot[j, i] > 0} for j, k in enumerate(self.topk)}

    def summarize(self, expected_ids=None):
        """-> FlickrEvaluator.summarize's dict: "Recall@1_all", "Recall@5_people", ..., "Upper_bound_all" (k = -1).  The raw report
        {k: {category: recall}} is kept in .results, as the reference keeps it.  expected_ids: (image_id, sentence_id) pairs that must
        have been seen; a missing one raises RuntimeError as the reference does."""
        self.results = self.report(expected_ids)
        score = {}
        for k, v in self.results.items():
            header = "Upper_bound" if k == -1 else f"Recall@{k}"
            for cat in sorted(v):
                score[f"{header}_{cat}"] = v[cat]
        return score


class RefExpPrecisionEvaluator(_RecallEvaluator):
    """RefExpEvaluator: precision@k by generalized IoU in fp32, per dataset name.  Targets: one phrase per image with its box as xyxy
    (the reference converts COCO's xywh as [x, y, w + x, h + y] in double) and "dataset_name"; pack them with
    pack_phrase_targets(samples, evaluator.datasets)."""
    MODE = 1

    def __init__(self, k=(1, 5, 10), thresh_iou=0.5, datasets=REFEXP_DATASETS):
        if any(int(x) <= 0 for x in k):
            raise ValueError(f"k {k}: positive entries")
        super().__init__(k, thresh_iou)
        self.datasets = tuple(datasets)

    def targets_for(self, samples, **kw):
        return pack_phrase_targets(samples, self.datasets, **kw)

    def summarize(self, expected_ids=None):
        """-> {dataset_name: sorted precisions over k} as RefExpEvaluator.summarize; a dataset without images scores 0.0."""
        pos, tot = self._counts(expected_ids)
        cats = self.categories or _categories(self.datasets)
        self.results = {}
        for name in self.datasets:
            i = cats.index(name)
            self.results[name] = sorted((float(pos[j, i]) / float(tot[j, i])) if tot[j, i] > 0 else 0.0 for j in range(len(self.topk)))
        return self.results


def evaluate_grounding(model, batches, evaluator, expected_ids=None):
    """The loop of engine/inference.py:483-575 for the grounding and refexp tasks, batched.  batches yields dicts with "images" (a
    DetImageList), "tokenizer_input", "positive_maps" (a list of B reference-form dicts, or PackedPositiveMaps on the device) and
    "targets" (PhraseTargets).  -> evaluator.summarize().  Nothing synchronises before summarize."""
    model.eval()
    with torch.no_grad():
        for batch in batches:
            images = batch["images"]
            detections = model(images, tokenizer_input=batch["tokenizer_input"], positive_map=batch["positive_maps"])
            boxes = images.boxes_to_original(detections)
            evaluator.update(boxes, detections, batch["targets"].to(boxes.device))
    return evaluator.summarize(expected_ids=expected_ids)
