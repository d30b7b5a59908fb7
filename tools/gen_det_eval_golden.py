"""Generate tests/golden/apeval_*.npz by executing the REFERENCE's LVIS evaluator on the CPU (runs where the reference tree is present):

    python tools/gen_det_eval_golden.py

Executed by path behind stub parents, unmodified: data/datasets/evaluation/lvis/lvis.py (LVIS, which holds no arithmetic) and
data/datasets/evaluation/lvis/lvis_eval.py (LVISResults, LVISEval, LvisEvaluatorFixedAP, convert_to_xywh).  Stand-ins without arithmetic:
`torchvision`, `torch._six`, `maskrcnn_benchmark.utils.mdetr_dist` (one process) and the parents of the relative imports.  The ONE stand-in
that carries arithmetic is `pycocotools.mask.iou` for boxes (see its docstring).

Inputs by name from tests/det_eval_cases.py; the fixtures hold outputs only: `precision`, `recall`, the `results` keys and values,
`num_gt`, and per detection slot `dt_matches != 0` / `dt_ignore` as the bits a * T + t of two uint64 words re-indexed to (image, slot),
with `kept` = the slots the reference evaluated.  Asserted and stored: every IoU of a same-category pair in an image differs from every
threshold by at least MARGIN except the pairs listed in EXACT, which must equal it; no two detections of one category share a score over
the whole case (the reference's tie order is an accident of list order); each case exercises what tests/det_eval_cases.py says it is
built for.  If a seed fails an assertion, change the seed, never the margin.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import shim                                      # noqa: E402
from tests import det_eval_cases as dv                       # noqa: E402

LV = os.path.join(shim.REF, "fine_grained", "maskrcnn_benchmark", "data", "datasets", "evaluation", "lvis")
OUT = os.path.join(ROOT, "tests", "golden")


def box_iou(dt, gt, iscrowd):
    """Stand-in for pycocotools.mask.iou on lists of [x, y, w, h] boxes: the box IoU of the COCO API without crowd (every iscrowd
    is 0 in lvis_eval.py:303).  THE ONE STAND-IN THAT CARRIES ARITHMETIC.  In double, per detection d and ground truth g:
        iw = max(min(dx + dw, gx + gw) - max(dx, gx), 0),  ih = max(min(dy + dh, gy + gh) - max(dy, gy), 0),  i = iw * ih
        iou = i / (dw * dh + gw * gh - i)
    -> array [len(dt), len(gt)]; [] when either list is empty, as the COCO API returns."""
    assert not any(iscrowd)
    if len(dt) == 0 or len(gt) == 0:
        return []
    out = np.zeros((len(dt), len(gt)), dtype=np.float64)
    for i, d in enumerate(dt):
        dx, dy, dw, dh = (np.float64(v) for v in d)
        for j, g in enumerate(gt):
            gx, gy, gw, gh = (np.float64(v) for v in g)
            iw = max(min(dx + dw, gx + gw) - max(dx, gx), np.float64(0))
            ih = max(min(dy + dh, gy + gh) - max(dy, gy), np.float64(0))
            inter = iw * ih
            out[i, j] = inter / (dw * dh + gw * gh - inter)
    return out


def load_reference():
    def pkg(name, **names):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in names.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m
    mb = "maskrcnn_benchmark"
    for n in (mb, mb + ".utils", mb + ".data", mb + ".data.datasets", mb + ".data.datasets.evaluation", mb + ".data.datasets.evaluation.lvis",
              "torchvision"):
        pkg(n)
    mask = pkg("pycocotools.mask", iou=box_iou)
    pkg("pycocotools", mask=mask)
    torch._six = pkg("torch._six")
    dist = pkg(mb + ".utils.mdetr_dist", is_main_process=lambda: True, all_gather=lambda x: [x])
    sys.modules[mb + ".utils"].mdetr_dist = dist
    shim._load("lvis", os.path.join(LV, "lvis.py"), mb + ".data.datasets.evaluation.lvis")
    return shim._load("lvis_eval", os.path.join(LV, "lvis_eval.py"), mb + ".data.datasets.evaluation.lvis")


def ground_truth(ref, k):
    """the case's annotations as an LVIS object (data only)"""
    gt = sys.modules[ref.LVIS.__module__].LVIS()
    anns = []
    for s in k["samples"]:
        for g, a in enumerate(s["annotations"]):
            anns.append(dict(a, image_id=s["image_id"], id=len(anns) + 1, index=g))
    gt.dataset = dict(images=[dict(id=s["image_id"], neg_category_ids=list(s["neg_category_ids"]),
                                   not_exhaustive_category_ids=list(s["not_exhaustive_category_ids"])) for s in k["samples"]],
                      categories=[dict(c) for c in k["categories"]], annotations=anns)
    gt._create_index()
    return gt


def predictions(k, images):
    """[(image_id, {"boxes", "scores", "labels"})] as the reference's inference loop hands them over (labels = category ids)"""
    det, ids = k["det"], [c["id"] for c in k["categories"]]
    out = []
    for b in images:
        n = int(det.count[b])
        out.append((k["samples"][b]["image_id"], dict(boxes=torch.from_numpy(det.boxes[b, :n].copy()), scores=torch.from_numpy(det.scores[b, :n].copy()),
                                                      labels=torch.tensor([ids[int(v) - 1] for v in det.labels[b, :n]], dtype=torch.int64))))
    return out


def run_standard(ref, k, gt):
    """prepare_for_lvis_detection's dicts (:694-716) with the slot as one more data field, LVISResults, LVISEval.run"""
    results = []
    for b, (image_id, p) in enumerate(predictions(k, range(len(k["samples"])))):
        boxes = ref.convert_to_xywh(p["boxes"]).tolist() if len(p["boxes"]) else []
        scores, labels = p["scores"].tolist(), p["labels"].tolist()
        results.extend(dict(image_id=image_id, category_id=labels[i], bbox=box, score=scores[i], slot=(b, i)) for i, box in enumerate(boxes))
    ev = ref.LVISEval(gt, ref.LVISResults(gt, results, max_dets=k["max_dets"]), iou_type="bbox")
    ev.params.max_dets = k["max_dets"]
    ev.run()
    return ev


def run_fixed(ref, k, gt):
    """LvisEvaluatorFixedAP fed in two updates; the LVISEval it builds inside _summarize_fixed is caught by a recording subclass"""
    made = []

    class Recording(ref.LVISEval):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    plain = ref.LVISEval
    ref.LVISEval = Recording
    try:
        ev = ref.LvisEvaluatorFixedAP(gt, topk=k["topk"], fixed_ap=True)
        B = len(k["samples"])
        for part in (range(0, B // 2), range(B // 2, B)):
            ev.update(predictions(k, part))
        ev.summarize()
    finally:
        ref.LVISEval = plain
    assert len(made) == 1
    return made[0]


def slot_of(k):
    """(image_id, category_id, score, bbox) -> (image, slot): the fixed-AP route builds its dicts itself"""
    det, ids = k["det"], [c["id"] for c in k["categories"]]
    table = {}
    for b, s in enumerate(k["samples"]):
        for d in range(int(det.count[b])):
            key = (s["image_id"], ids[int(det.labels[b, d]) - 1], float(det.scores[b, d]), float(det.boxes[b, d, 0]), float(det.boxes[b, d, 1]))
            assert key not in table
            table[key] = (b, d)
    return table


def check_inputs(case, k, ev):
    det = k["det"]
    for ci in range(len(k["categories"])):
        s = [float(det.scores[b, d]) for b in range(len(det.count)) for d in range(int(det.count[b])) if det.labels[b, d] == ci + 1]
        assert len(set(s)) == len(s), f"{case}: two detections of category {ci} share a score"
    image = {s["image_id"]: b for b, s in enumerate(k["samples"])}
    margin, exact = np.inf, []
    for (img_id, _), ious in ev.ious.items():
        for v in np.asarray(ious, np.float64).reshape(-1):
            gap = np.abs(v - ev.params.iou_thrs)
            if gap.min() < dv.MARGIN:
                assert gap.min() == 0, f"{case}: an IoU within {gap.min():.2e} of a threshold: change the seed"
                exact.append((image[img_id], float(v)))
            else:
                margin = min(margin, float(gap.min()))
    assert sorted(exact) == sorted((e[0], e[3]) for e in dv.EXACT[case]), f"{case}: IoUs on a threshold {exact}, built for {dv.EXACT[case]}"
    return margin


def generate(ref, case):
    k = dv.case_inputs(case)
    gt = ground_truth(ref, k)
    ev = run_fixed(ref, k, gt) if k["topk"] is not None else run_standard(ref, k, gt)
    p = ev.params
    assert np.array_equal(p.iou_thrs, dv.IOU_THRS) and np.array_equal(p.rec_thrs, dv.REC_THRS) and np.array_equal(np.asarray(p.area_rng, np.float64), dv.AREA_RNG)
    assert p.cat_ids == [c["id"] for c in k["categories"]]
    margin = check_inputs(case, k, ev)
    B, D = k["det"].labels.shape
    T, A, C, I = len(p.iou_thrs), len(p.area_rng), len(p.cat_ids), len(p.img_ids)
    match, ignore, kept = np.zeros((B, D), np.uint64), np.zeros((B, D), np.uint64), np.zeros((B, D), np.uint8)
    num_gt = np.zeros((C, A), np.int64)
    lookup = slot_of(k)
    assert len(ev.eval_imgs) == C * A * I
    for ci in range(C):
        for a in range(A):
            for ii in range(I):
                e = ev.eval_imgs[(ci * A + a) * I + ii]
                if e is None:
                    continue
                num_gt[ci, a] += int(np.count_nonzero(np.asarray(e["gt_ignore"]) == 0))
                for j, dt_id in enumerate(e["dt_ids"]):
                    ann = ev.lvis_dt.anns[dt_id]
                    slot = tuple(ann["slot"]) if "slot" in ann else lookup[(ann["image_id"], ann["category_id"], ann["score"], ann["bbox"][0], ann["bbox"][1])]
                    kept[slot] = 1
                    for t in range(T):
                        bit = np.uint64(1) << np.uint64(a * T + t)
                        if e["dt_matches"][t, j] != 0:
                            match[slot] |= bit
                        if e["dt_ignore"][t, j]:
                            ignore[slot] |= bit
    precision, recall = ev.eval["precision"], ev.eval["recall"]
    results = {key: v for key, v in ev.results.items() if k["topk"] is None or key.startswith("AP")}
    built_for(case, k, match, ignore, kept, num_gt, precision, results)
    np.savez_compressed(os.path.join(OUT, case + ".npz"), precision=precision, recall=recall, results_keys=np.array(list(results)),
                        results_vals=np.array([float(v) for v in results.values()], np.float64), num_gt=num_gt, match=match, ignore=ignore,
                        kept=kept, margin_iou=np.float64(margin))
    print(case, "margin", f"{margin:.3e}", "records", int(kept.sum()), {key: round(float(v), 4) for key, v in results.items()})


def built_for(case, k, match, ignore, kept, num_gt, precision, results):
    """each case exercises what tests/det_eval_cases.py says it is built for"""
    det = k["det"]
    T = len(dv.IOU_THRS)
    every = np.uint64((1 << T) - 1)                          # area range "all"
    inside = np.zeros_like(kept, bool)
    for b, n in enumerate(det.count):
        inside[b, :n if k["max_dets"] < 0 or k["topk"] is not None else min(int(n), k["max_dets"])] = True
    assert int(kept.sum()) > 0 and int((match[kept == 1] != 0).sum()) > 0 and int((match[kept == 1] == 0).sum()) > 0
    if case == "apeval_small":
        assert all(results[key] > -1 for key in ("APr", "APc", "APf")), "all three frequency groups are evaluated"
    if case == "apeval_edge":
        assert int((inside & (kept == 0)).sum()) == 1, "one detection dropped by the federated filter"
        assert int(det.count[5]) - k["max_dets"] == 2 and not kept[5, 4:].any(), "two detections cut by max_dets"
        assert kept[0, :2].all() and (match[0, :2] == 0).all() and (ignore[0, :2] & every == 0).all(), "false positives of a negative category"
        assert kept[2, 2] and match[2, 2] == 0 and ignore[2, 2] & every == every, "unmatched, not exhaustive: ignored"
        won = np.uint64(sum(1 << t for t in range(T) if dv.IOU_THRS[t] < 0.82))
        assert match[3, 0] & every == every and ignore[3, 0] & every == every & ~won, "the non-ignored one wins where it qualifies"
        assert match[3, 1] & every == ignore[3, 1] & every != 0, "only an ignored ground truth qualifies: ignored"
        assert match[4, 0] & every == np.uint64(sum(1 << t for t in range(T) if dv.IOU_THRS[t] < 0.777)), "7/9"
        assert match[4, 2] & every == np.uint64(sum(1 << t for t in range(T) if dv.IOU_THRS[t] < 0.86)), "the next detection gets the earlier one"
        assert match[4, 1] & every == np.uint64(1), "IoU = 1/2 matches at 0.5 and nowhere else"
        assert num_gt[3].tolist() == [3, 1, 3, 1], "areas of 32^2 and 96^2 count in both neighbouring ranges"
        assert (precision[:, :, 5, 0] == 0).all() and (precision[:, :, 6, :] == -1).all() and results["APr"] == -1
    if case == "apeval_wide":
        assert int(((det.labels == 1) & (kept == 1)).sum()) >= 192 and int(((det.labels[0] == 1) & (kept[0] == 1)).sum()) > 64
        assert sum(1 for a in k["samples"][0]["annotations"] if a["category_id"] == k["categories"][0]["id"]) > 64
    if case == "apeval_fixed":
        per_cat = [int(((det.labels == ci + 1) & inside).sum()) for ci in range(len(k["categories"]))]
        assert sum(1 for n in per_cat if n > k["topk"]) >= 2, "several categories are truncated"
        assert det.scores[0, 0] == np.float32(0.995) and not kept[0, 0], "truncated in, then dropped by the federated filter"
        top = int(det.labels[0, 0])
        assert per_cat[top - 1] > k["topk"] and int(((det.labels == top) & (kept == 1)).sum()) <= k["topk"] - 1, \
            "the dropped record had taken one of the k places"


def main():
    torch.set_num_threads(8)
    ref = load_reference()
    for case in dv.CASES:
        generate(ref, case)


if __name__ == "__main__":
    main()
