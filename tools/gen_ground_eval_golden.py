"""Generate tests/golden/geval_*.npz by executing the REFERENCE's grounding evaluators on the CPU (runs where the reference tree is present):

    python tools/gen_ground_eval_golden.py

Executed by path behind stub parents, unmodified: engine/inference.py (flickr_post_process, resize_box), structures/bounding_box.py,
data/datasets/evaluation/flickr/flickr_eval.py (FlickrEvaluator, Flickr30kEntitiesRecallEvaluator, box_iou, _merge_boxes, the Flickr30k
Entities readers), data/datasets/refexp.py (RefExpEvaluator) and layers/set_loss.py (generalized_box_iou).  Stand-ins, none of which
carries arithmetic: `prettytable.PrettyTable` (a table that is printed and dropped), the `dist` helpers (one process), the parents of
the relative imports, and a duck-typed object for the COCO API that RefExpEvaluator reads its targets from (data only).

The Flickr evaluator reads its ground truth from a Flickr30k Entities directory: one is written to a temporary folder from
tests/ground_eval_cases.py (test.txt, Annotations/<id>.xml, Sentences/<id>.txt) and read back by the reference's own parsers.

Inputs by name from tests/ground_eval_cases.py (the fixtures hold outputs only): the reference's report and score keys, its per-phrase
hits, and per-phrase `best` from the reference's box_iou / generalized_box_iou on the reference's own post-processed boxes.  Asserted
and stored: every best differs from the threshold by at least the case's margin, except the listed exact-threshold phrases, which must
equal it; no two detections of an image share a score (torch.topk / sorted tie order is undefined in the reference); the layout gives the
hits tests/ground_eval_cases.py says it is built to give.  If a seed fails a margin, change the seed, never the margin.

RefExpEvaluator raises on an image without detections (the empty zip, refexp.py:61): the reference is run on the images that have
some, and the fixture says which.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import shim                                      # noqa: E402
from tests import ground_eval_cases as ge                    # noqa: E402

MB = os.path.join(shim.REF, "fine_grained", "maskrcnn_benchmark")
OUT = os.path.join(ROOT, "tests", "golden")


class _Table:
    field_names = ()

    def add_row(self, row):
        pass

    def __str__(self):
        return "(table)"


def load_reference():
    def pkg(name, **names):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in names.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m
    one = dict(is_main_process=lambda: True, all_gather=lambda x: [x], synchronize=lambda: None)
    mb = "maskrcnn_benchmark"
    for n in (mb, mb + ".structures", mb + ".data", mb + ".data.datasets", mb + ".data.datasets.evaluation.flickr", mb + ".utils", mb + ".engine"):
        pkg(n)
    pkg("prettytable", PrettyTable=_Table)
    pkg(mb + ".data.datasets.evaluation", evaluate=None, im_detect_bbox_aug=None)
    pkg(mb + ".data.datasets.modulated_coco", ModulatedDataset=type("ModulatedDataset", (), {}))
    pkg(mb + ".layers", nms=None, ml_nms=None)
    for n in ("comm", "mdetr_dist", "dist"):
        pkg(f"{mb}.utils.{n}", **one)
    bb = shim._load("bounding_box", os.path.join(MB, "structures", "bounding_box.py"), mb + ".structures")
    shim._load("boxlist_ops", os.path.join(MB, "structures", "boxlist_ops.py"), mb + ".structures")
    sl = shim._load("set_loss", os.path.join(MB, "layers", "set_loss.py"), mb + ".layers")
    fe = shim._load("flickr_eval", os.path.join(MB, "data", "datasets", "evaluation", "flickr", "flickr_eval.py"), mb + ".data.datasets.evaluation.flickr")
    rx = shim._load("refexp", os.path.join(MB, "data", "datasets", "refexp.py"), mb + ".data.datasets")
    inf = shim._load("inference", os.path.join(MB, "engine", "inference.py"), mb + ".engine")
    return types.SimpleNamespace(BoxList=bb.BoxList, set_loss=sl, flickr=fe, refexp=rx, inference=inf)


def write_flickr_dir(root, samples):
    """A Flickr30k Entities directory holding `samples`: phrase p of an image is entity p + 1"""
    os.makedirs(os.path.join(root, "Annotations"))
    os.makedirs(os.path.join(root, "Sentences"))
    with open(os.path.join(root, "test.txt"), "w") as f:
        f.write("\n".join(s["image_id"] for s in samples) + "\n")
    for s in samples:
        objs, words = [], []
        for p, ph in enumerate(s["phrases"]):
            for x1, y1, x2, y2 in ph["boxes"]:
                objs.append(f"<object><name>{p + 1}</name><bndbox><xmin>{x1}</xmin><ymin>{y1}</ymin><xmax>{x2}</xmax><ymax>{y2}</ymax></bndbox></object>")
            words.append(f"[/EN#{p + 1}/{'/'.join(ph['phrase_type'])} phrase number {p + 1}] and")
        w, h = ge.FRAME
        with open(os.path.join(root, "Annotations", s["image_id"] + ".xml"), "w") as f:
            f.write(f"<annotation><size><width>{w}</width><height>{h}</height><depth>3</depth></size>{''.join(objs)}</annotation>")
        with open(os.path.join(root, "Sentences", s["image_id"] + ".txt"), "w") as f:
            f.write(" ".join(words) + " nothing else .\n")


def check_scores(det):
    gap = np.inf
    for b, n in enumerate(det.count.tolist()):
        s = det.scores[b, :n]
        assert len(set(s.tolist())) == n, f"image {b}: two detections share a score"
        if n > 1:
            gap = min(gap, float(np.abs(np.diff(np.sort(s.astype(np.float64)))).min()))
    return gap


def check_margin(case, best, live, mode):
    """live: bool [B, P] (phrases that exist and were evaluated) -> the smallest |best - thresh| outside the exact phrases"""
    m = np.inf
    for b, p in zip(*np.nonzero(live)):
        d = np.abs(best[b, p] - ge.THRESH)
        if (int(b), int(p)) in ge.EXACT[case]:
            assert (d == 0).all(), f"{case} ({b}, {p}): built to sit on the threshold exactly, best {best[b, p]}"
        else:
            m = min(m, float(d.min()))
    assert m >= ge.MARGINS[mode], f"{case}: a best within {m:.2e} of the threshold (< {ge.MARGINS[mode]:.0e}): change the seed"
    return m


def flat_report(rep):
    ks, cats, vals = [], [], []
    for k, row in rep.items():
        for c, v in row.items():
            ks.append(int(k)), cats.append(str(c)), vals.append(float(v))
    return dict(report_k=np.array(ks, np.int64), report_cat=np.array(cats), report_val=np.array(vals, np.float64))


def generate_flickr(ref, case):
    det, samples, _, topk, _, merge = ge.case_inputs(case)
    B, P, K = len(samples), max(len(s["phrases"]) for s in samples), len(topk)
    gap = check_scores(det)
    with tempfile.TemporaryDirectory() as root:
        write_flickr_dir(root, samples)
        ev = ref.flickr.FlickrEvaluator(root, "test", top_k=topk, iou_thresh=ge.THRESH, merge_boxes=merge)
    preds = []
    w, h = ge.FRAME
    for b, s in enumerate(samples):
        n = int(det.count[b])
        out = ref.BoxList(torch.from_numpy(det.boxes[b, :n].copy()), (w, h), mode="xyxy")
        out.add_field("scores", torch.from_numpy(det.scores[b, :n].copy()))
        out.add_field("labels", torch.from_numpy(det.labels[b, :n].astype(np.int64)))
        tgt = ref.BoxList(torch.zeros((0, 4)), (w, h), mode="xyxy")
        tgt.add_field("orig_size", torch.tensor([h, w]))
        tgt.add_field("original_img_id", s["image_id"])
        tgt.add_field("sentence_id", s["sentence_id"])
        preds.append(ref.inference.flickr_post_process(out, [tgt], {p + 1: [p] for p in range(len(s["phrases"]))}, 1))
    ev.update(preds)
    score = ev.summarize()
    rep = ev.results
    best, hit, live = np.zeros((B, P, K)), np.zeros((B, P, K), np.int32), np.zeros((B, P), bool)
    inner = ev.evaluator
    for b, (s, pred) in enumerate(zip(samples, preds)):
        phrases = inner.imgid2sentences[s["image_id"]][0]
        assert len(phrases) == len(s["phrases"]) == len(pred["boxes"])
        for p, (cur, ph) in enumerate(zip(pred["boxes"], phrases)):
            ious = ref.flickr.box_iou(np.asarray(cur), np.asarray(inner.imgid2boxes[s["image_id"]][ph["phrase_id"]]))
            for j, k in enumerate(topk):
                best[b, p, j] = ious.max() if k == -1 else ious[:k].max()
            hit[b, p] = best[b, p] >= ge.THRESH
            live[b, p] = True
    margin = check_margin(case, best, live, 0)
    if not merge:
        for (b, p), want in ge.FLICKR_EXPECT.items():
            assert tuple(hit[b, p].tolist()) == want, f"{case} ({b}, {p}): built to hit {want}, the reference says {hit[b, p].tolist()}"
    # the report follows from the per-phrase hits: the reference's tally and ours of its IoUs agree
    for j, k in enumerate(topk):
        assert abs(rep[k]["all"] - hit[live][:, j].mean()) < 1e-15
    np.savez_compressed(os.path.join(OUT, case + ".npz"), best=best, hit=hit, live=live, score_keys=np.array(list(score)),
                        score_vals=np.array(list(score.values()), np.float64), margin_thresh=np.float64(margin), margin_scores=np.float64(gap),
                        **flat_report(rep))
    print(case, "margin", f"{margin:.3e}", "score gap", f"{gap:.3e}", {k: round(v, 4) for k, v in score.items() if k.endswith("_all")})


class _RefExpGT:
    """What RefExpEvaluator reads of the COCO API: imgs, getAnnIds, loadImgs, loadAnns (one annotation per image)"""

    def __init__(self, samples):
        self.imgs = {s["image_id"]: {"dataset_name": s["dataset_name"]} for s in samples}
        self.anns = {s["image_id"]: {"bbox": list(s["bbox_xywh"])} for s in samples}

    def getAnnIds(self, imgIds):
        return [imgIds]

    def loadImgs(self, i):
        return [self.imgs[i]]

    def loadAnns(self, i):
        return [self.anns[i]]


def generate_refexp(ref, case):
    det, samples, datasets, topk, _, _ = ge.case_inputs(case)
    B, K = len(samples), len(topk)
    gap = check_scores(det)
    with_det = [b for b in range(B) if det.count[b] > 0]
    ev = ref.refexp.RefExpEvaluator(_RefExpGT([samples[b] for b in with_det]), ("bbox",), k=topk, thresh_iou=ge.THRESH)
    best, hit, live = np.zeros((B, 1, K)), np.zeros((B, 1, K), np.int32), np.zeros((B, 1), bool)
    for b in with_det:
        n = int(det.count[b])
        scores, boxes = torch.from_numpy(det.scores[b, :n].copy()), torch.from_numpy(det.boxes[b, :n].copy())
        ev.update({samples[b]["image_id"]: {"scores": scores, "boxes": boxes}})
        ordered = sorted(zip(scores.tolist(), boxes.tolist()), reverse=True)
        sb = torch.cat([torch.as_tensor(x).view(1, 4) for _, x in ordered])
        giou = ref.set_loss.generalized_box_iou(sb, torch.as_tensor(ge.refexp_xyxy(samples[b]["bbox_xywh"])).view(-1, 4))
        assert giou.dtype == torch.float32
        for j, k in enumerate(topk):
            best[b, 0, j] = float(max(giou[:k]))
        hit[b, 0] = best[b, 0].astype(np.float32) >= np.float32(ge.THRESH)
        live[b, 0] = True
    results = ev.summarize()
    margin = check_margin(case, best, live, 1)
    for b, want in ge.REFEXP_EXPECT.items():
        if b in with_det:
            assert tuple(hit[b, 0].tolist()) == want, f"{case} image {b}: built to hit {want}, the reference says {hit[b, 0].tolist()}"
    assert float(best[live].min()) < 0, "the case holds a negative GIoU"
    for d in datasets:                                        # the reference's tally and ours of its GIoUs agree
        mine = [b for b in with_det if samples[b]["dataset_name"] == d]
        assert results[d] == sorted(float(np.mean([hit[b, 0, j] for b in mine])) if mine else 0.0 for j in range(K)), (d, results[d])
    np.savez_compressed(os.path.join(OUT, case + ".npz"), best=best, hit=hit, live=live, ref_images=np.array(with_det, np.int64),
                        results_name=np.array(list(results)), results_val=np.array([results[d] for d in results], np.float64),
                        margin_thresh=np.float64(margin), margin_scores=np.float64(gap))
    print(case, "margin", f"{margin:.3e}", "score gap", f"{gap:.3e}", results)


def main():
    torch.set_num_threads(8)
    ref = load_reference()
    for case, c in ge.CASES.items():
        (generate_flickr if c["mode"] == 0 else generate_refexp)(ref, case)


if __name__ == "__main__":
    main()
