"""Time box AP evaluation on the device: one BoxAPEvaluator.update at B = 8, D = 300, C = 1203 (one launch of fiber_ap_match, no
synchronisation) and the tables of `--records` records (two stable sorts, then one launch of fiber_ap_accumulate), beside the host loop the
reference runs (tests/det_eval_cases.restate_match / restate_accumulate on the same inputs: a device-to-host copy, then Python / numpy
scalars; the benchmark does not depend on the reference tree).

    python tools/det_eval_bench.py [--iters 200] [--records 6000000] [--host-records 60000]

Device timing: device events around back-to-back calls after a warm-up, 5 windows: median, minimum and maximum.  The host loops are timed
with time.perf_counter, once each (they take seconds); the accumulation restatement runs on --host-records records only and says so.
Prints one JSON line.  Nothing here is asserted as a ratio."""
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

import det_eval_cases as dv                                   # noqa: E402
from fiber_amd import ops                                     # noqa: E402
from fiber_amd.modules.detection_eval import BoxAPEvaluator, pack_detection_targets   # noqa: E402

B, D, C, GT = 8, 300, 1203, 40
T, A = len(dv.IOU_THRS), len(dv.AREA_RNG)


def make(seed=0):
    g = np.random.default_rng(seed)
    cats = [dict(id=i + 1, frequency="rcf"[i % 3]) for i in range(C)]
    samples, boxes, labels = [], np.zeros((B, D, 4), np.float32), np.zeros((B, D), np.int32)
    for b in range(B):
        present = g.choice(C, 12, replace=False)
        anns = []
        for _ in range(GT):
            x, y, w, h = g.uniform(0, 500), g.uniform(0, 400), g.uniform(10, 200), g.uniform(10, 200)
            anns.append(dict(bbox=[float(x), float(y), float(w), float(h)], area=float(w * h * g.uniform(0.6, 1.0)), category_id=int(present[g.integers(12)]) + 1))
        neg = [int(c) + 1 for c in g.choice(C, 40, replace=False) if c not in present]
        samples.append(dict(image_id=b, annotations=anns, neg_category_ids=neg, not_exhaustive_category_ids=[int(present[0]) + 1]))
        for d in range(D):
            if d % 2 == 0:
                a = anns[g.integers(GT)]
                x, y, w, h = a["bbox"]
                e = g.uniform(-0.15, 0.15, 4) * np.array([w, h, w, h])
                boxes[b, d], labels[b, d] = [x + e[0], y + e[1], x + w + e[2], y + h + e[3]], a["category_id"]
            else:
                x, y = g.uniform(0, 500), g.uniform(0, 400)
                boxes[b, d], labels[b, d] = [x, y, x + g.uniform(10, 200), y + g.uniform(10, 200)], int(g.choice(neg + [int(present[1]) + 1]))
    scores = -np.sort(-g.permutation(B * D).reshape(B, D).astype(np.float32) / (B * D + 1), axis=1)
    return cats, samples, types.SimpleNamespace(boxes=boxes, scores=scores, labels=labels, count=np.full((B,), D, np.int32))


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
    return [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--records", type=int, default=6_000_000)
    ap.add_argument("--host-records", type=int, default=60_000)
    a = ap.parse_args()
    cats, samples, det = make()
    targets = pack_detection_targets(samples, cats).to("cuda")
    dev = types.SimpleNamespace(**{k: torch.from_numpy(v).cuda() for k, v in vars(det).items()})
    ev = BoxAPEvaluator(cats)

    def update():
        ev.reset()
        return ev.update(dev, targets)
    match, ignore, valid = update()
    t0 = time.perf_counter()
    r = dv.restate_match(dict(categories=cats, samples=samples, det=det, max_dets=300, topk=None))
    host_match_s = time.perf_counter() - t0
    res = {"B": B, "D": D, "C": C, "G": int(targets.gt.shape[1]), "T": T, "A": A,
           "same_match": bool(np.array_equal(match.cpu().numpy().view(np.uint64), r["match"]) and np.array_equal(ignore.cpu().numpy().view(np.uint64), r["ignore"])
                              and np.array_equal(valid.cpu().numpy(), r["valid"])),
           "device_update_ms_med_min_max": windows(update, a.iters), "host_restate_match_s": round(host_match_s, 3)}

    g = torch.Generator(device="cuda").manual_seed(0)
    N = a.records
    big = BoxAPEvaluator(cats)
    big.update(dev, targets)                                 # allocates the state
    big.reset()
    hit = torch.randint(0, 1 << 40, (N,), generator=g, device="cuda", dtype=torch.int64)
    big._records = [(torch.rand(N, generator=g, device="cuda"), torch.randint(1, C + 1, (N,), generator=g, device="cuda", dtype=torch.int32), hit,
                     hit & torch.randint(0, 1 << 40, (N,), generator=g, device="cuda", dtype=torch.int64),
                     torch.ones(N, dtype=torch.uint8, device="cuda"), torch.ones(N, dtype=torch.bool, device="cuda"))]
    big.num_gt += torch.randint(1, 4000, big.num_gt.shape, generator=g, device="cuda")

    def tables():
        big._tables = None
        return big.tables()
    res["records"] = N
    res["device_tables_ms_med_min_max"] = windows(tables, 3)
    scores, labels, m, ig, _, _ = big._records[0]
    order, cats_sorted = big._ordered(scores, labels.long() - 1)
    seg = torch.searchsorted(cats_sorted, torch.arange(C + 1, device="cuda"))
    ms, igs = m[order].contiguous(), ig[order].contiguous()
    res["device_accumulate_kernel_ms_med_min_max"] = windows(lambda: ops.ap_accumulate(ms, igs, seg, big.num_gt, big._rec, T), 5)

    n = min(a.host_records, N)
    sub = BoxAPEvaluator(cats)
    sub.update(dev, targets)
    sub.reset()
    sub._records = [tuple(col[:n] for col in big._records[0])]
    sub.num_gt += big.num_gt
    precision, recall = sub.tables()
    hs, hl = scores[:n].cpu().numpy(), labels[:n].cpu().numpy()
    hm, hi = m[:n].cpu().numpy().view(np.uint64), ig[:n].cpu().numpy().view(np.uint64)
    t0 = time.perf_counter()
    records = [sorted(np.nonzero(hl == c + 1)[0].tolist(), key=lambda i: -float(hs[i])) for c in range(C)]
    hp, hr = dv.restate_accumulate(records, hm, hi, big.num_gt.cpu().numpy(), T)
    res["host_records"] = n
    res["host_restate_accumulate_s"] = round(time.perf_counter() - t0, 3)
    res["same_tables"] = bool(np.array_equal(precision.cpu().numpy(), hp) and np.array_equal(recall.cpu().numpy(), hr))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
