"""Generate tests/golden/detect_*.npz by executing the REFERENCE's grounding post-processing on the CPU (runs where the reference tree is present):

    python tools/gen_detect_golden.py            # the committed seeds of tests/detect_cases.py; asserts the margins
    python tools/gen_detect_golden.py --search   # per case, the first seed (of a few hundred) whose margins hold, then the same

Executed by path behind stub parents, unmodified: modeling/rpn/inference.py (ATSSPostProcessor, convert_grounding_to_od_logits[_v2]),
modeling/box_coder.py, modeling/rpn/anchor_generator.py, modeling/utils.py, structures/bounding_box.py, structures/image_list.py and
structures/boxlist_ops.py.

The ONE stand-in is the compiled NMS (the extension cannot be built here): `maskrcnn_benchmark._C.ml_nms` becomes a few lines of greedy
NMS -- sort by descending score, devIoU with the +1 convention and equal labels, strict >, kept indices returned ascending, as
csrc/cuda/ml_nms.cu does.  It stands in for `_C.ml_nms` and not, as one might expect on a CPU, for `_C.nms`: boxlist_ml_nms's CPU branch
(structures/boxlist_ops.py:55-66) appends each label's keep indices WITHOUT mapping them back through that label's subset, so it selects
unrelated boxes; what the model computes is the branch taken on a GPU.  boxlist_ops' device test is steered there by giving that module a
view of `torch` whose `device("cpu")` compares unequal; every line executed is the reference's.

Inputs by name from tests/detect_cases.py (the product regenerates them identically; the fixtures hold outputs only).  Discrete outputs are
only comparable where the reference itself is decisive, so everything is also evaluated in fp64 (detect_cases.postprocess_torch) and the
margins of detect_cases.MARGINS are asserted and stored: every agg against the threshold, the score gap across every top-k cut and across
the D cut, consecutive sorted final scores, every same-label IoU among the sorted candidates against NMS_TH, and the fp32 reference
keep-set against the fp64 keep-set.  `source{b}` (level, anchor, class of each detection) is not something the reference computes: it
is taken from the fp64 restatement's detections, which are tied to the reference's rows by equal count, equal labels in score order and
boxes within 1e-2 (asserted here); scores, boxes, labels and anchors in the fixtures are the reference's own.  Where no seed satisfies them the case's pre_nms_top_n is lowered in detect_cases.py, never the margins.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import shim                                      # noqa: E402
from tests import detect_cases as dc                         # noqa: E402

MB = os.path.join(shim.REF, "fine_grained", "maskrcnn_benchmark")
OUT = os.path.join(ROOT, "tests", "golden")


def _dev_iou(a, b):
    """devIoU (ml_nms.cu:15-26) on two rows (x1, y1, x2, y2, score, label) of numpy float32 scalars, in its operation order.  Written out
    here on purpose: the stand-in shares no arithmetic with tests/detect_cases.py, whose restatement the fixtures are to judge."""
    one, zero = np.float32(1), np.float32(0)
    if a[5] != b[5]:
        return zero
    left, right = max(a[0], b[0]), min(a[2], b[2])
    top, bottom = max(a[1], b[1]), min(a[3], b[3])
    width, height = max(right - left + one, zero), max(bottom - top + one, zero)
    inter = width * height
    sa = (a[2] - a[0] + one) * (a[3] - a[1] + one)
    sb = (b[2] - b[0] + one) * (b[3] - b[1] + one)
    return inter / (sa + sb - inter)


def ml_nms_standin(boxes, scores, labels, thresh):
    """csrc/cuda/ml_nms.cu on the CPU, scalar by scalar in fp32: -> ascending original indices of the kept boxes"""
    order = np.argsort(-scores.numpy(), kind="stable")
    rows = np.concatenate([boxes.numpy()[order], scores.numpy()[order, None], labels.numpy()[order, None]], axis=1).astype(np.float32)
    thresh = np.float32(thresh)
    n = len(rows)
    removed = np.zeros(n, dtype=bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(order[i])
        for j in range(i + 1, n):
            if not removed[j] and _dev_iou(rows[i], rows[j]) > thresh:
                removed[j] = True
    return torch.as_tensor(sorted(int(k) for k in keep), dtype=torch.long)


class _TorchView:
    """`torch` for boxlist_ops alone: device(...) never equals a tensor's device, so boxlist_ml_nms takes its GPU branch"""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def device(*_a):
        return object()


def load_reference():
    def pkg(name):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
        return m
    for n in ("maskrcnn_benchmark", "maskrcnn_benchmark.structures", "maskrcnn_benchmark.modeling", "maskrcnn_benchmark.modeling.rpn"):
        pkg(n)
    c = pkg("maskrcnn_benchmark._C")
    c.ml_nms = ml_nms_standin
    layers = pkg("maskrcnn_benchmark.layers")
    layers.ml_nms = c.ml_nms
    layers.nms = None                                        # (only boxlist_nms and the unusable CPU branch call it)
    s, m = "maskrcnn_benchmark.structures", "maskrcnn_benchmark.modeling"
    shim._load("bounding_box", os.path.join(MB, "structures", "bounding_box.py"), s)
    shim._load("image_list", os.path.join(MB, "structures", "image_list.py"), s)
    ops = shim._load("boxlist_ops", os.path.join(MB, "structures", "boxlist_ops.py"), s)
    ops.torch = _TorchView()
    shim._load("box_coder", os.path.join(MB, "modeling", "box_coder.py"), m)
    shim._load("utils", os.path.join(MB, "modeling", "utils.py"), m)
    ag = shim._load("anchor_generator", os.path.join(MB, "modeling", "rpn", "anchor_generator.py"), m + ".rpn")
    inf = shim._load("inference", os.path.join(MB, "modeling", "rpn", "inference.py"), m + ".rpn")
    return inf, ag, sys.modules[m + ".box_coder"], sys.modules[s + ".image_list"]


def margins(case, seed=None):
    """fp64 evaluation -> (dict of achieved margins, the fp64 result)"""
    c = dc.CASES[case]
    r = dc.run_case(case, torch.float64, seed=seed)
    agg = min(float((a[:, :, [int(k) - 1 for k in c["positive_map"]]] - c["thresh"]).abs().min()) for a in r["agg"])
    cut = min(float((v[:, -1] - rest)[v[:, -1] >= 0].min()) if bool((v[:, -1] >= 0).any()) else float("inf") for v, rest in zip(r["topk"], r["rest"]))
    s = r["cand_scores"]
    kept_sorted = min(float((r["scores"][b, :n - 1] - r["scores"][b, 1:n]).min()) if n > 1 else float("inf")
                      for b, n in enumerate(r["count"].tolist()))
    dcut = float("inf")                                       # gap between the last kept and the next survivor the D cut leaves out
    allkeep = dc.greedy_keep(r["sup"], s, s.shape[1])
    for b in range(s.shape[0]):
        ks = s[b][allkeep[b]]
        if len(ks) > c["D"]:
            dcut = min(dcut, float(ks[c["D"] - 1] - ks[c["D"]]))
    iou = dc.iou_matrix(r["cand_boxes"])
    pair = (r["cand_labels"][:, :, None] == r["cand_labels"][:, None, :]) & (s >= 0)[:, :, None] & (s >= 0)[:, None, :]
    pair &= torch.triu(torch.ones(pair.shape[1:], dtype=torch.bool), 1)
    ioum = float((iou[pair] - c["nms"]).abs().min())
    return dict(agg_vs_thresh=agg, cut_gap=min(cut, dcut), sorted_gap=kept_sorted, iou_vs_nms=ioum,
                survivors=[int(k.sum()) for k in allkeep], candidates=[int((s[b] >= 0).sum()) for b in range(s.shape[0])]), r


def margins_ok(m):
    return all(m[k] >= v for k, v in dc.MARGINS.items())


def run_reference(ref, case):
    inf, ag, bc, il = ref
    c = dc.CASES[case]
    cfg = dc.cfg_for(case)
    x = dc.inputs(case)
    post = inf.make_atss_postprocessor(cfg, bc.BoxCoder((10.0, 10.0, 5.0, 5.0)), is_train=False)
    gen = ag.make_anchor_generator_complex(cfg)
    H, W = max(h for _, h in c["image_sizes"]), max(w for w, _ in c["image_sizes"])
    images = il.ImageList(torch.zeros(c["B"], 3, H, W), [(h, w) for w, h in c["image_sizes"]])
    anchors = gen(images, x["bbox_reg"])
    box_cls = [torch.zeros(c["B"], c["C"], h, w) for h, w in c["sizes"]]               # its channel count is all the v1 mapping reads
    with torch.no_grad():
        res = post(x["bbox_reg"], x["centerness"], anchors, box_cls, None, x["logits"], c["positive_map"])
    return res, [a.bbox for a in anchors[0]]


def generate(ref, case):
    c = dc.CASES[case]
    m, r64 = margins(case)
    print(case, {k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in m.items()})
    assert margins_ok(m), f"{case}: margins {m} below {dc.MARGINS}"
    res, anchors = run_reference(ref, case)
    rec = {"anchors%d" % l: a.numpy() for l, a in enumerate(anchors)}
    for b, bl in enumerate(res):
        rec[f"boxes{b}"], rec[f"scores{b}"] = bl.bbox.numpy(), bl.get_field("scores").numpy()
        rec[f"labels{b}"] = bl.get_field("labels").numpy().astype(np.int64)
        # the fp32 reference keep-set against the fp64 keep-set: the same (score-ordered) labels, and boxes that agree to fp32 rounding
        n = int(r64["count"][b])
        order = np.argsort(-rec[f"scores{b}"], kind="stable")
        assert len(order) == n, (case, b, len(order), n)
        assert np.array_equal(rec[f"labels{b}"][order], r64["labels"][b, :n].numpy()), f"{case} image {b}: fp32 and fp64 keep-sets differ"
        assert np.allclose(rec[f"boxes{b}"][order], r64["boxes"][b, :n].numpy(), rtol=0, atol=1e-2), f"{case} image {b}: fp32 and fp64 keep-sets differ"
        rec[f"source{b}"] = r64["source"][b, :n].numpy()[np.argsort(order)]            # source of each reference row (reference order)
    for k in dc.MARGINS:
        rec["margin_" + k] = np.float64(m[k])
    rec["survivors"], rec["candidates"] = np.array(m["survivors"]), np.array(m["candidates"])
    np.savez_compressed(os.path.join(OUT, case + ".npz"), **rec)
    print(case, "detections", [len(bl) for bl in res], "survivors before the D cut", m["survivors"], "candidates", m["candidates"])


def search(case, tries=300):
    for seed in range(tries):
        m, _ = margins(case, seed)
        ok = margins_ok(m)
        print(case, "seed", seed, {k: f"{m[k]:.2e}" for k in dc.MARGINS}, m["survivors"], m["candidates"], "OK" if ok else "")
        if ok:
            return seed
    raise SystemExit(f"{case}: no seed below {tries} satisfies the margins: lower its pre_nms_top_n")


def main():
    torch.set_num_threads(8)
    if "--search" in sys.argv:
        for case in dc.CASES:
            print(case, "-> seed", search(case))
        return
    ref = load_reference()
    for case in dc.CASES:
        generate(ref, case)


if __name__ == "__main__":
    main()
