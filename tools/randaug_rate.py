"""Throughput of the coarse-grained TRAINING transform on the device, at the per-GPU batch of a training step: 256 camera-sized sources
(480 x 640 uint8) -> 384 x 384, ImageNet mean / std.

  (a) data.DeviceRandAugTransform (RandomResizedCrop + flip + RandomAugment(2, 7) + ToTensor + Normalize): warm-up, then --rounds rounds of
      --calls calls, each call with a fresh seed (so the drawn ops change from call to call), each round between two events on the
      stream and ending in a synchronise; images/s per round, the median and the spread over the rounds.  The host part of a call (the
      plan and the tables, python) is inside the timed window: it is reported on its own as well.
  (b) data.DeviceImageTransform (the validation transform: resize + ToTensor + Normalize) on the same sources in the same process, its
      rounds alternating with (a)'s.
--profile (a run of its own, the profiler slows the host): the device time of every kernel of 10 calls with torch.profiler, per launch.

    python tools/randaug_rate.py [--batch 256] [--rounds 7] [--calls 10] [--profile]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fiber_amd import data, lib  # noqa: E402

DEV = "cuda"
H, W, S, SEED = 480, 640, 384, 1234


def spread(v):
    return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1), "rounds": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "randaug_rate needs a HIP device"
    lib.load()
    B = args.batch
    rng = np.random.default_rng(0)
    base = [torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(DEV) for _ in range(8)]
    dev = [base[i % 8] for i in range(B)]                             # 8 distinct sources: 7 MB, far beyond nothing but fewer H2D copies
    aug, val = data.DeviceRandAugTransform(S), data.DeviceImageTransform(S)
    seeds = iter(range(SEED, SEED + 10 ** 6))
    res = {"batch": B, "source": [H, W], "size": S, "out_bytes": B * 3 * S * S * 4}

    def call_aug():
        return aug(dev, next(seeds))

    def call_val():
        return val(dev)

    calls = []
    real = lib.call
    lib.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    call_aug()
    res["abi_calls_per_batch"] = list(calls)
    lib.call = real
    for _ in range(3):
        call_aug()
        call_val()
    torch.cuda.synchronize()

    if args.profile:
        from torch.profiler import ProfilerActivity, profile

        def kernels(fn, n=10):
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(n):
                    fn()
                torch.cuda.synchronize()
            acc = {}
            for e in prof.events():
                if e.device_type == torch.autograd.DeviceType.CUDA:
                    dur = getattr(e, "device_time", None)
                    dur = e.cuda_time if dur is None else dur
                    acc.setdefault(e.name.replace("(anonymous namespace)::", "").split("(")[0].strip(), []).append(float(dur))
            return {k: {"launches_per_batch": len(v) / n, "median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1),
                        "max_us": round(max(v), 1), "sum_us_per_batch": round(sum(v) / n, 1)} for k, v in acc.items()}

        for name, fn in (("randaug", call_aug), ("validation", call_val)):
            res[f"kernels_{name}"] = kernels(fn)
            res[f"device_us_per_batch_{name}"] = round(sum(v["sum_us_per_batch"] for v in res[f"kernels_{name}"].values()), 1)
            for k, v in sorted(res[f"kernels_{name}"].items()):
                print(f"  [{name}] {k[:56]:56s} x{v['launches_per_batch']:.1f}  median {v['median_us']:9.1f} us  (min {v['min_us']:.1f}, "
                      f"max {v['max_us']:.1f})  per batch {v['sum_us_per_batch']:9.1f} us")
        print(json.dumps(res))
        return

    def rounds(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.calls):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return B * args.calls / (start.elapsed_time(stop) * 1e-3)

    rates = {"randaug": [], "validation": []}
    for _ in range(args.rounds):                                      # alternate: both see the same neighbours on the machine
        rates["randaug"].append(rounds(call_aug))
        rates["validation"].append(rounds(call_val))
    res["images_per_s"] = {k: spread(v) for k, v in rates.items()}
    shapes = [(H, W)] * B
    t0 = time.perf_counter()
    for k in range(5):
        aug.plan(shapes, SEED + k)
    res["host_plan_ms_per_batch"] = round((time.perf_counter() - t0) / 5 * 1e3, 2)
    p = aug.plan(shapes, SEED)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(5):
        aug.apply(dev, p)
    res["host_apply_enqueue_ms_per_batch"] = round((time.perf_counter() - t0) / 5 * 1e3, 2)      # returns before the kernels finish
    torch.cuda.synchronize()
    res["ms_per_batch"] = {k: round(B / v["median"] * 1e3, 3) for k, v in res["images_per_s"].items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
