"""Time one phrase-grounding evaluator update at B = 8, D = 100, P = 8, G = 3: PhraseRecallEvaluator.update on the device (one launch of
fiber_ground_recall, no synchronisation) against the host loop the reference runs per sentence (tests/ground_eval_cases.restate on the same
detections: a device-to-host copy of the Detections, then Python / numpy scalars), and against the package's own numpy path on CPU tensors.

    python tools/ground_eval_bench.py [--iters 2000] [--mode 0|1]

Timing of the device path: device events around `iters` back-to-back updates after a warm-up, 7 such windows: median, minimum and maximum
per update.  The host paths are timed with time.perf_counter around whole updates (they end on the host), the copy of the detections
included, 5 runs each.  Prints one JSON line.  Nothing here is asserted as a ratio."""
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

import ground_eval_cases as ge                                # noqa: E402
from fiber_amd.modules.grounding_eval import PhraseRecallEvaluator, RefExpPrecisionEvaluator   # noqa: E402

B, D, P, G = 8, 100, 8, 3


def make(mode, seed=0):
    g = np.random.default_rng(seed)
    P_ = P if mode == 0 else 1
    xy = g.uniform(0, 500, (B, D, 2))
    wh = g.uniform(20, 140, (B, D, 2))
    boxes = np.concatenate([xy, xy + wh], -1).astype(np.float32)
    labels = g.integers(1, P_ + 1, (B, D)).astype(np.int32)
    count = np.array([D, D - 7, 64, 37, D, 90, 1, D], np.int32)
    samples = []
    for b in range(B):
        phrases = []
        for p in range(P_):
            n = 1 if mode == 1 else 1 + (b + p) % G
            src = boxes[b, g.integers(0, D, n)].astype(np.float64)
            phrases.append(dict(boxes=[[float(np.floor(s[0])), float(np.floor(s[1])), float(np.ceil(s[2])) + 1, float(np.ceil(s[3])) + 1] for s in src],
                                phrase_type=[] if mode == 1 else [ge.FLICKR_CATEGORIES[(b + p) % 8]]))
        samples.append(dict(image_id=b, sentence_id=0, phrases=phrases, **({"dataset_name": ge.REFEXP_DATASETS[b % 3]} if mode == 1 else {})))
    return boxes, labels, count, samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--mode", type=int, default=0, choices=(0, 1))
    a = ap.parse_args()
    boxes, labels, count, samples = make(a.mode)
    new = (lambda: PhraseRecallEvaluator()) if a.mode == 0 else (lambda: RefExpPrecisionEvaluator())     # noqa: E731
    ev = new()
    cats = ge.FLICKR_CATEGORIES if a.mode == 0 else ge.REFEXP_DATASETS
    host_t = ev.targets_for(samples, cats) if a.mode == 0 else ev.targets_for(samples)
    dev_t = host_t.to("cuda")
    det = types.SimpleNamespace(boxes=torch.from_numpy(boxes).cuda(), labels=torch.from_numpy(labels).cuda(), count=torch.from_numpy(count).cuda())

    def device():
        ev.evaluated_ids.clear()                             # the same batch again: not a repeat
        return ev.update(det.boxes, det, dev_t)

    hit, _ = device()
    r = ge.restate(boxes, labels, count, samples, ev.topk, 0.5, a.mode)
    res = {"mode": a.mode, "B": B, "D": D, "P": hit.shape[1], "G": int(host_t.gt.shape[2]), "K": len(ev.topk),
           "same_hits": bool(np.array_equal(hit.cpu().numpy(), r["hit"]))}
    torch.cuda.synchronize()
    ts = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            device()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / a.iters)
    res["device_update_ms"] = round(statistics.median(ts), 4)
    res["device_update_ms_min_max"] = [round(min(ts), 4), round(max(ts), 4)]

    def host_loop():                                         # what the reference does: detections to the host, then a Python loop
        hb, hl, hc = det.boxes.cpu().numpy(), det.labels.cpu().numpy(), det.count.cpu().numpy()
        return ge.restate(hb, hl, hc, samples, ev.topk, 0.5, a.mode)

    cpu_ev = new()

    def host_numpy():                                        # the package's CPU path on a host copy of the detections
        cpu_ev.evaluated_ids.clear()
        ns = types.SimpleNamespace(labels=det.labels.cpu(), count=det.count.cpu())
        return cpu_ev.update(det.boxes.cpu(), ns, host_t)

    for name, fn in (("host_loop", host_loop), ("host_numpy", host_numpy)):
        fn()
        tt = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            tt.append((time.perf_counter() - t0) * 1e3)
        res[name + "_ms"] = round(statistics.median(tt), 3)
        res[name + "_ms_min_max"] = [round(min(tt), 3), round(max(tt), 3)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
