"""Time chunked open-vocabulary detection: GeneralizedVLRCNN.detect_chunked (the image prefix once per batch, the text prefix once per
evaluation, the fused rest on pair batches of P prompts, one merge launch) beside the naive loop of one whole-model call per chunk, which is
what the model could do per chunk before.

    python tools/chunked_det_bench.py [--reps 5] [--height 800] [--width 1344] [--chunks 8] [--passes 1,2,4,8]
    python tools/chunked_det_bench.py --sensitivity [--height H --width W]    the batch-size sensitivity the pair-batch test is bounded by
    python tools/chunked_det_bench.py --head-repeat        which outputs of VLDyHead are not the same bits on every execution

Setup: Swin-B depths (2, 2, 18, 2), B = 2 images, K chunks of 40 categories, DETECTIONS_PER_IMG 300, PRE_NMS_TOP_N 3000, six tower
convolutions; random weights (the work does not depend on them; bias0 is zeroed so that NMS has candidates to walk).  The variants alternate
inside one process after a warm-up of each; a call is timed with device events and ends in a synchronise.  Reported per variant: median,
minimum and maximum over --reps, and the peak of torch's allocator during the call.  The merge kernel alone is timed at [2, 31, 300]
(back-to-back launches in 5 windows).  Prints one JSON line.  No ratio is asserted.

--sensitivity runs the backbone forward AS IT STOOD BEFORE THE SPLIT (tests/chunk_cases.forward_unsplit, the parent's code operation for
operation) at the pair-batch test's shapes on the replicated batch and on plain batches of B, and prints the largest rel-L2 distance per
output: the value recorded as chunk_cases.BATCH_SENSITIVITY."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import chunk_cases as cc                                      # noqa: E402
import fpn_cases as fc                                        # noqa: E402
from fiber_amd import ops                                     # noqa: E402

DEV = "cuda"


def sensitivity(height, width):
    model = cc.make_detector((2, 2, 18, 2), DEV)
    prompts = cc.pair_prompts().to(DEV)
    images, _ = cc.pair_inputs(DEV)
    if (height, width) != (cc.PAIR["H"], cc.PAIR["W"]):
        images = torch.from_numpy(np.random.default_rng(5).standard_normal((cc.PAIR["B"], 3, height, width)).astype(np.float32)).to(DEV)
    fb = model.fusion_backbone
    with torch.no_grad():
        runs = [cc.batch_sensitivity(lambda t, x: cc.forward_unsplit(fb, t, x), images, prompts, cc.PAIR["P"]) for _ in range(2)]
        split = cc.batch_sensitivity(fb, images, prompts, cc.PAIR["P"])
    assert runs[0] == runs[1], "the measurement is not repeatable"
    print(json.dumps({"shape": dict({k: cc.PAIR[k] for k in ("B", "chunk", "P")}, H=height, W=width), "BATCH_SENSITIVITY": runs[0],
                      "split_forward": split}))


def head_repeat(n=4):
    """VLDyHead on the same features n times: which of its outputs are not the same bits every time"""
    model = cc.make_detector((2, 2, 2, 2), DEV)
    prompts = cc.pair_prompts().to(DEV)
    images, _ = cc.pair_inputs(DEV)
    fb, head = model.fusion_backbone, model.rpn.head
    names = {0: "cls_logits", 1: "bbox_reg", 2: "centerness", 6: "dot_product_logits"}
    with torch.no_grad():
        ii, ti = cc.pair_indices(cc.PAIR["B"], 0, cc.PAIR["P"], DEV)
        visual, lang, _ = fb.fuse(fb.image_prefix(images), fb.text_prefix({"input_ids": prompts.input_ids, "attention_mask": prompts.attention_mask}), ii, ti)
        runs = [head(list(visual), lang, lang["embedded"]) for _ in range(n)]
    diff = {}
    for a, b in zip(runs, runs[1:]):
        for i, name in names.items():
            for level, (x, y) in enumerate(zip(a[i], b[i])):
                if not torch.equal(x, y):
                    d = diff.setdefault(f"{name}[{level}]", {"shape": list(x.shape), "max_abs": 0.0, "elements": 0})
                    d["max_abs"] = max(d["max_abs"], float((x - y).abs().max()))
                    d["elements"] = max(d["elements"], int((x != y).sum()))
    print(json.dumps({"head_runs": n, "outputs_that_differ_between_runs": diff}))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def merge_kernel_time(iters=200, n=5):
    x = cc.merge_inputs("lvis")
    dev = [t.to(DEV) for t in cc.merge_args(x)[:6]]
    out = ops.det_merge(*dev, 300)

    def fn():
        ops.det_merge(*dev, 300, out=out)
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        ts.append(timed(lambda: [fn() for _ in range(iters)])[0] / iters)
    return [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sensitivity", action="store_true")
    ap.add_argument("--head-repeat", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--height", type=int)
    ap.add_argument("--width", type=int)
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--passes", default="1,2,4,8")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if a.head_repeat:
        return head_repeat()
    if a.sensitivity:
        return sensitivity(a.height or cc.PAIR["H"], a.width or cc.PAIR["W"])
    a.height, a.width = a.height or 800, a.width or 1344
    from fiber_amd.modules import GeneralizedVLRCNN, build_detection_prompts
    B, K, Cc = 2, a.chunks, 40
    torch.manual_seed(0)
    cfg = fc.model_cfg(depths=(2, 2, 18, 2), convs=6, **{"MODEL.ATSS.DETECTIONS_PER_IMG": 300, "MODEL.ATSS.PRE_NMS_TOP_N": 3000,
                                                        "TEST.MDETR_STYLE_AGGREGATE_CLASS_NUM": Cc})
    model = GeneralizedVLRCNN(cfg)
    with torch.no_grad():
        model.rpn.head.bias0.zero_()
    model = model.to(DEV).eval()
    cats = [dict(id=i + 1, name=f"thing{i} kind") for i in range(K * Cc)]
    prompts = build_detection_prompts(cats, cc.StubTokenizer(), chunk=Cc).to(DEV)
    g = np.random.default_rng(0)
    images = torch.from_numpy(g.standard_normal((B, 3, a.height, a.width)).astype(np.float32)).to(DEV)
    sizes = torch.tensor([[float(a.width), float(a.height)], [float(a.width - 44), float(a.height - 30)]], device=DEV)
    tok = [{"input_ids": prompts.input_ids[k:k + 1].expand(B, -1).contiguous(), "attention_mask": prompts.attention_mask[k:k + 1].expand(B, -1).contiguous()}
           for k in range(K)]
    maps = [prompts.positive_maps[k] for k in range(K)]

    def naive():
        """one whole-model call per chunk, then the same merge"""
        dets = [model((images, sizes), tokenizer_input=tok[k], positive_map=maps[k]) for k in range(K)]
        cols = [torch.stack([getattr(d, f) for d in dets], dim=1) for f in ("boxes", "scores", "labels", "source", "count")]
        return ops.det_merge(*cols, prompts.label_table, 300)

    with torch.no_grad():
        state = model.encode_prompts(prompts)
        variants = {"naive": naive}
        for P in [int(p) for p in a.passes.split(",")]:
            variants[f"chunked_P{P}"] = (lambda P=P: model.detect_chunked((images, sizes), state, prompts_per_pass=P, max_dets=300))
        res = {"B": B, "K": K, "Cc": Cc, "image": [a.height, a.width], "reps": a.reps}
        peak, outs = {}, {}
        for name, fn in variants.items():                    # warm-up, peak memory, and the result for the comparison below
            torch.cuda.reset_peak_memory_stats()
            _, outs[name] = timed(fn)
            peak[name] = round(torch.cuda.max_memory_allocated() / 2 ** 20)
        times = {name: [] for name in variants}
        for _ in range(a.reps):
            for name, fn in variants.items():
                times[name].append(timed(fn)[0])
        res["text_prefix_ms"] = round(statistics.median([timed(lambda: model.encode_prompts(prompts))[0] for _ in range(3)]), 3)
    ref = outs["naive"]
    for name in variants:
        o = outs[name]
        o = o if isinstance(o, tuple) else (o.boxes, o.scores, o.labels, o.source, o.chunk, o.count)
        same = float((o[2] == ref[2]).float().mean())
        res[name] = {"ms_med_min_max": [round(statistics.median(times[name]), 2), round(min(times[name]), 2), round(max(times[name]), 2)],
                     "peak_MiB": peak[name], "labels_equal_to_naive": round(same, 4), "count": o[5].tolist(),
                     "score_rel_l2_to_naive": float(f"{fc.rel_l2(o[1], ref[1]):.3e}")}
    res["merge_kernel_ms_med_min_max_2x31x300"] = merge_kernel_time()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
