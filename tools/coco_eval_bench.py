"""Time COCO-protocol box AP on the device: one CocoBoxEvaluator.update at a COCO-val-shaped batch, B = 8, D = 100, C = 80, 20 ground
truths per image over 6 categories, one in ten crowd (one launch of fiber_ap_match_coco, no synchronisation), and tables + summarize at
`--images` images' worth of records (per max_dets two stable sorts and one launch of fiber_ap_accumulate, then the one copy), beside the
scalar restatement of the matching on the same batch (tests/coco_eval_cases.restate_match: Python / numpy scalars on the host).  The
restatement is a Python restatement of COCOeval.evaluateImg, NOT pycocotools, which is not available here: PARITY UNPINNED against the
pycocotools binary, and no figure below says anything about its speed.

    python tools/coco_eval_bench.py [--iters 200] [--images 5000]

Device timing: device events around back-to-back calls after a warm-up, 5 windows: median, minimum and maximum.  tables + summarize ends
in a device-to-host copy and is timed with time.perf_counter around synchronised calls.  The host loop is timed once.  Prints one JSON
line.  Nothing here is asserted as a ratio."""
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

import coco_eval_cases as cv                                  # noqa: E402
from fiber_amd.modules.detection_eval import CocoBoxEvaluator, pack_coco_targets   # noqa: E402

B, D, C, GT, PRESENT = 8, 100, 80, 20, 6


def make(seed=0):
    g = np.random.default_rng(seed)
    cats = [dict(id=i + 1) for i in range(C)]
    samples, boxes, labels = [], np.zeros((B, D, 4), np.float32), np.zeros((B, D), np.int32)
    for b in range(B):
        present = g.choice(C, PRESENT, replace=False)
        anns = []
        for i in range(GT):
            x, y, w, h = g.uniform(0, 500), g.uniform(0, 400), g.uniform(10, 200), g.uniform(10, 200)
            anns.append(dict(bbox=[float(x), float(y), float(w), float(h)], area=float(w * h * g.uniform(0.6, 1.0)),
                             category_id=int(present[g.integers(PRESENT)]) + 1, iscrowd=1 if i % 10 == 9 else 0))
        samples.append(dict(image_id=b, annotations=anns))
        for d in range(D):
            if d % 2 == 0:
                a = anns[g.integers(GT)]
                x, y, w, h = a["bbox"]
                e = g.uniform(-0.15, 0.15, 4) * np.array([w, h, w, h])
                boxes[b, d], labels[b, d] = [x + e[0], y + e[1], x + w + e[2], y + h + e[3]], a["category_id"]
            else:
                x, y = g.uniform(0, 500), g.uniform(0, 400)
                boxes[b, d], labels[b, d] = [x, y, x + g.uniform(10, 200), y + g.uniform(10, 200)], int(g.integers(C)) + 1
    scores = -np.sort(-g.permutation(B * D).reshape(B, D).astype(np.float32) / (B * D + 1), axis=1)
    return cats, samples, types.SimpleNamespace(boxes=boxes, scores=scores, labels=labels, count=np.full((B,), D, np.int32))


def spread(ts):
    return [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)]


def windows(fn, iters, n=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / iters)
    return spread(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--images", type=int, default=5000)
    a = ap.parse_args()
    cats, samples, det = make()
    targets = pack_coco_targets(samples, cats).to("cuda")
    dev = types.SimpleNamespace(**{k: torch.from_numpy(v).cuda() for k, v in vars(det).items()})
    ev = CocoBoxEvaluator(cats)

    def update():
        ev.reset()
        return ev.update(dev, targets)
    match, ignore, rank, valid = update()
    k = dict(categories=cats, samples=samples, det=det, max_dets=(1, 10, 100))
    t0 = time.perf_counter()
    r = cv.restate_match(k, 1)
    host_match_s = time.perf_counter() - t0
    same = np.array_equal(match.cpu().numpy().view(np.uint64), r["match"]) and np.array_equal(ignore.cpu().numpy().view(np.uint64), r["ignore"]) \
        and np.array_equal(valid.cpu().numpy(), r["valid"]) and np.array_equal(rank.cpu().numpy(), r["rank"]) \
        and np.array_equal(ev.num_gt.cpu().numpy(), r["num_gt"])
    res = {"B": B, "D": D, "C": C, "G": int(targets.gt.shape[1]), "T": cv.T, "A": cv.A, "same_match": bool(same),
           "device_update_ms_med_min_max": windows(update, a.iters), "host_restate_match_s": round(host_match_s, 3)}

    g = torch.Generator(device="cuda").manual_seed(0)
    N = a.images * D
    big = CocoBoxEvaluator(cats)
    big.update(dev, targets)                                 # allocates the state
    big.reset()
    hit = torch.randint(0, 1 << 40, (N,), generator=g, device="cuda", dtype=torch.int64)
    big._records = [(torch.rand(N, generator=g, device="cuda"), torch.randint(1, C + 1, (N,), generator=g, device="cuda", dtype=torch.int32), hit,
                     hit & torch.randint(0, 1 << 40, (N,), generator=g, device="cuda", dtype=torch.int64),
                     torch.ones(N, dtype=torch.uint8, device="cuda"), torch.randint(0, 12, (N,), generator=g, device="cuda", dtype=torch.int32))]
    big.num_gt += torch.randint(1, 4000, big.num_gt.shape, generator=g, device="cuda")

    def summary():
        big._tables = None
        return big.summarize()
    summary()
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        summary()
        ts.append((time.perf_counter() - t0) * 1e3)
    res["images"], res["records"] = a.images, N
    res["tables_summarize_ms_med_min_max"] = spread(ts)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
