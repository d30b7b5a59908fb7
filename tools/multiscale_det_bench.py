"""Time the merge of multi-scale test-time augmentation: ops.det_aug_collect (one launch per view) + ops.det_aug_merge (one int64 sort, the
per-class merge kernel, one sort by score and gathers) on the device beside the numpy path of the SAME ops calls, and the merge's share of
a whole GeneralizedVLRCNN.detect_multiscale.

    python tools/multiscale_det_bench.py [--reps 5] [--host-reps 1] [--views 24] [--per-view 5000] [--skip-model]

Synthetic candidates: B = 2 images, --views views x --per-view candidates each (the reference's default protocol is 12 TEST.SCALES x FLIP
= 24 views of 5 levels x PRE_NMS_TOP_N 1000); --per-view objects per image with uniform labels, each seen in every view with a jitter of
+-3 pixels and its own score, 2 % padding; views alternate un-flipped / flipped, ratio 3 / 2.  Sizes: "lvis" 1203 classes, "coco" 80.
Both TEST.SPECIAL_NMS modes at TH 0.5, PRE_NMS_TOP_N 1000 (what the reference's configs cut to).  Device calls are timed with events
around the whole call after a warm-up, --reps times, variants alternating in one process; the host path with perf_counter.  Reported:
median, minimum, maximum in ms.  The model part runs a (2, 2, 6, 2) Swin (Swin-T's depths at the widths the fused backbone hard-wires) on
two 480 x 640 images over 6 scales x flip and times detect_multiscale as a whole and collect + merge replayed on its own candidates.
Prints one JSON line.  No ratio is asserted."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fiber_amd import ops                                     # noqa: E402

DEV = "cuda"
FRAME = (800, 1200)                                          # the original (H, W); the views are 1200 x 1800


def synthetic(B, views, per_view, classes, seed=0):
    """-> per view (boxes [B, n, 4] in the view's frame, scores, labels, source) on the host, and the per-view rows"""
    g = np.random.default_rng(seed)
    H, W = FRAME
    oh, ow = H * 3 // 2, W * 3 // 2
    w, h = g.integers(20, 300, (B, per_view)), g.integers(20, 300, (B, per_view))
    x, y = (g.random((B, per_view)) * (W - w - 8)).astype(np.int64) + 4, (g.random((B, per_view)) * (H - h - 8)).astype(np.int64) + 4
    labels = g.integers(1, classes + 1, (B, per_view)).astype(np.int32)
    out = []
    for v in range(views):
        j = g.integers(-3, 4, (4, B, per_view))
        box = np.stack((x + j[0], y + j[1], x + w + j[2], y + h + j[3]), axis=-1).astype(np.float32) * np.float32(1.5)
        flip = bool(v % 2)
        if flip:
            box[..., 0], box[..., 2] = ow - 1 - box[..., 2], ow - 1 - box[..., 0]
        scores = g.random((B, per_view)).astype(np.float32) * 0.9 + 0.05
        scores[g.random((B, per_view)) < 0.02] = -1.0
        source = g.integers(0, 1 << 28, (B, per_view)).astype(np.int32)
        rows = ops.det_aug_view_rows([FRAME] * B, [(oh, ow)] * B, flip, None)
        out.append(([torch.from_numpy(a) for a in (box, scores, labels, source)], rows))
    return out


def pipeline(views, classes, mode, top_n, device):
    B, T = views[0][0][1].shape[0], sum(v[0][1].shape[1] for v in views)
    cand = [[t.to(device) for t in c] for c, _ in views]
    cls = torch.arange(1, classes + 1, dtype=torch.int32, device=device)

    def run():
        out = (torch.empty((B, T, 4), dtype=torch.float32, device=device), torch.empty((B, T), dtype=torch.float32, device=device),
               torch.empty((B, T), dtype=torch.int32, device=device), torch.empty((B, T), dtype=torch.int32, device=device),
               torch.empty((B, T), dtype=torch.int32, device=device))
        off = 0
        for v, (c, (_, rows)) in enumerate(zip(cand, views)):
            ops.det_aug_collect(*c, rows, cls, out, off, v)
            off += c[1].shape[1]
        return ops.det_aug_merge(*out, cls, 0.5, mode, top_n)
    return run


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def stats(ts):
    return [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)]


def model_share(reps):
    import chunk_cases as cc
    import det_input_cases as di
    import fpn_cases as fc
    from fiber_amd import data
    from fiber_amd.modules import GeneralizedVLRCNN
    torch.manual_seed(0)
    cfg = di.input_cfg(fc.model_cfg(depths=(2, 2, 6, 2), convs=6, **{"MODEL.ATSS.PRE_NMS_TOP_N": 1000, "TEST.MDETR_STYLE_AGGREGATE_CLASS_NUM": 80}),
                       divisible=32)
    model = GeneralizedVLRCNN(cfg)
    with torch.no_grad():
        model.rpn.head.bias0.zero_()
    model = model.to(DEV).eval()
    g = np.random.default_rng(1)
    images = [torch.from_numpy(g.integers(0, 256, (480, 640, 3), dtype=np.uint8)).to(DEV) for _ in range(2)]
    tok = cc.StubTokenizer()
    ids = [torch.tensor([0] + [tok.word_id(f"thing{i}") for i in range(80)] + [2])] * 2
    tokens = {k: v.to(DEV) for k, v in data.pad_input_ids(ids, 256, True).items()}
    pmap = {c + 1: [c + 1] for c in range(80)}
    test = types.SimpleNamespace(SCALES=(400, 500, 600, 700, 800, 900), RANGES=(), MAX_SIZE=1500, FLIP=True, SPECIAL_NMS="vote", TH=0.5,
                                 PRE_NMS_TOP_N=1000, NUM_CLASSES=81, SELECT_CLASSES=())
    seen, real = [], ops.det_aug_collect

    def record(*a):
        seen.append(a)
        return real(*a)
    ops.det_aug_collect = record
    try:
        _, det = timed(lambda: model.detect_multiscale(images, tokenizer_input=tokens, positive_map=pmap, test_cfg=test))
    finally:
        ops.det_aug_collect = real
    cls, T = seen[0][5], seen[0][6][1].shape[1]

    def merge_only():
        out = tuple(torch.empty_like(t) for t in seen[0][6])
        for a in seen:
            ops.det_aug_collect(*a[:6], out, a[7], a[8])
        return ops.det_aug_merge(*out, cls, 0.5, "vote", 1000)
    merge_only()
    whole, part = [], []
    for _ in range(reps):
        whole.append(timed(lambda: model.detect_multiscale(images, tokenizer_input=tokens, positive_map=pmap, test_cfg=test))[0])
        part.append(timed(merge_only)[0])
    return {"views": len(seen), "T": int(T), "count": det.count.tolist(), "detect_multiscale_ms": stats(whole), "collect_merge_ms": stats(part),
            "share": round(statistics.median(part) / statistics.median(whole), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--per-view", type=int, default=5000)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    res = {"B": 2, "views": a.views, "per_view": a.per_view, "T": a.views * a.per_view, "reps": a.reps, "top_n": 1000}
    runs = {}
    for name, classes in (("lvis", 1203), ("coco", 80)):
        views = synthetic(2, a.views, a.per_view, classes)
        for mode in ("none", "vote"):
            runs[f"{name}_{mode}"] = (pipeline(views, classes, mode, 1000, DEV), pipeline(views, classes, mode, 1000, "cpu"))
    times = {k: [] for k in runs}
    outs = {k: timed(dev)[1] for k, (dev, _) in runs.items()}                    # warm-up
    for _ in range(a.reps):
        for k, (dev, _) in runs.items():
            times[k].append(timed(dev)[0])
    for k, (_, host) in runs.items():
        ht = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            want = host()
            ht.append((time.perf_counter() - t0) * 1e3)
        same = bool(torch.equal(outs[k][1].cpu(), want[1]) and torch.equal(outs[k][2].cpu(), want[2]) and torch.equal(outs[k][5].cpu(), want[5]))
        res[k] = {"device_ms_med_min_max": stats(times[k]), "numpy_ms_med_min_max": stats(ht), "count": outs[k][5].tolist(),
                  "scores_labels_equal_to_numpy": same, "box_max_abs_diff": float((outs[k][0].cpu() - want[0]).abs().max())}
    if not a.skip_model:
        with torch.no_grad():
            res["model"] = model_share(a.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
