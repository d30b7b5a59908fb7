"""Throughput of the grounding input pipeline on one batch of 8 camera-sized sources (480 x 640 uint8 -> min_size 800 / max_size 1333,
"bgr255", divisibility 32: the FIBER yamls' training input):
  (a) data.DeviceDetectionTransform on the device: warm-up, then --rounds rounds of --calls calls, each round between two events on the
      stream; images/s per round, the median and the spread over the rounds; the launch count of one call
  (b) one host loader worker doing the same work with PIL + torch on ONE thread (resize, flip, to-tensor, normalise, pad)
--profile (a run of its own, the profiler slows the host): the device time of each kernel of one call with torch.profiler, the share of
the fused second pass against the horizontal pass, and the second pass against the HBM-write time of the padded tensor.

    python tools/det_input_bench.py [--rounds 7] [--calls 20] [--profile] [--no-host]"""
import argparse
import json
import os
import statistics
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fiber_amd import data, lib  # noqa: E402

HBM_PEAK = 8.0e12     # bytes/s (MI355X_MICROARCH.md)
DEV = "cuda"
MEAN, STD = (103.530, 116.280, 123.675), (57.375, 57.120, 58.395)
B, H, W, MIN_SIZE, MAX_SIZE, SEED = 8, 480, 640, 800, 1333, 1234


def cfg():
    ns = types.SimpleNamespace
    return ns(INPUT=ns(MIN_SIZE_TRAIN=(MIN_SIZE,), MAX_SIZE_TRAIN=MAX_SIZE, MIN_SIZE_TEST=MIN_SIZE, MAX_SIZE_TEST=MAX_SIZE, PIXEL_MEAN=list(MEAN),
                       PIXEL_STD=list(STD), FORMAT="", TO_BGR255=True, FIX_RES=False),
              AUGMENT=ns(MULT_MIN_SIZE_TRAIN=(), FLIP_PROB_TRAIN=0.5, VERTICAL_FLIP_PROB_TRAIN=0.0), DATALOADER=ns(SIZE_DIVISIBILITY=32))


def host_worker(images, sizes, flips, pad):
    """What one loader worker of the reference does per batch: build_transforms per sample, then to_image_list"""
    from PIL import Image
    mean, std = torch.tensor(MEAN)[:, None, None], torch.tensor(STD)[:, None, None]
    per = []
    for im, (oh, ow), f in zip(images, sizes, flips):
        r = Image.fromarray(im, "RGB").resize((ow, oh), Image.BILINEAR)
        if f:
            r = r.transpose(Image.FLIP_LEFT_RIGHT)
        t = torch.from_numpy(np.array(r)).permute(2, 0, 1).float().div(255)
        t = t[[2, 1, 0]] * 255
        per.append(t.sub_(mean).div_(std))
    out = per[0].new_zeros((len(per), 3) + tuple(pad))
    for p, o in zip(per, out):
        o[:, :p.shape[1], :p.shape[2]].copy_(p)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "det_input_bench needs a HIP device"
    lib.load()
    rng = np.random.default_rng(0)
    host = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(B)]
    dev = [torch.from_numpy(im).to(DEV) for im in host]
    t = data.DeviceDetectionTransform(cfg(), is_train=True)
    sizes, flips, pad = t.plan([(H, W)] * B, SEED)
    out_bytes = B * 3 * pad[0] * pad[1] * 4
    res = {"batch": B, "source": [H, W], "image_sizes": sizes, "flips": flips, "padded": list(pad), "out_bytes": out_bytes}

    def call():
        return t(dev, SEED)

    for _ in range(5):
        call()
    torch.cuda.synchronize()

    if args.profile:
        from torch.profiler import ProfilerActivity, profile

        def kernels(fn):
            fn()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(10):
                    fn()
                torch.cuda.synchronize()
            acc = {}
            for e in prof.events():
                if e.device_type == torch.autograd.DeviceType.CUDA:
                    dur = getattr(e, "device_time", None)
                    dur = e.cuda_time if dur is None else dur
                    acc.setdefault(e.name.replace("(anonymous namespace)::", "").split("(")[0].strip(), []).append(float(dur))
            return {k: {"calls_per_batch": len(v) / 10, "median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in acc.items()}

        kern = kernels(call)
        res["kernels"] = kern
        # the same canvas with nothing inside it: 8 sources of 8 x 8 kept at 8 x 8, every wave of the second pass but one per image on the
        # padding path (stores only) -- what this grid shape costs when it only writes
        tiny = [torch.zeros((8, 8, 3), dtype=torch.uint8, device=DEV) for _ in range(B)]
        t_pad = data.DeviceDetectionTransform(cfg(), is_train=False)
        t_pad.padded_shape = lambda sizes: pad
        res["kernels_all_padding"] = kernels(lambda: t_pad.apply(tiny, [(8, 8)] * B, [False] * B))
        h = next((v["median_us"] for k, v in kern.items() if "det_h_kernel" in k), None)
        v2 = next((v["median_us"] for k, v in kern.items() if "det_v_norm_pad_kernel" in k), None)
        vp = next((v["median_us"] for k, v in res["kernels_all_padding"].items() if "det_v_norm_pad_kernel" in k), None)
        if h and v2:
            res["second_pass_share_of_both_passes"] = v2 / (h + v2)
            res["second_pass_us"], res["horizontal_pass_us"], res["second_pass_all_padding_us"] = v2, h, vp
            res["hbm_write_floor_us"] = {"at_8.0_TBps_peak": out_bytes / HBM_PEAK * 1e6, "at_6.3_TBps_achievable": out_bytes / 6.3e12 * 1e6}
            res["second_pass_write_rate_TBps"] = out_bytes / (v2 * 1e-6) / 1e12
        for name, kk in (("batch", kern), ("all padding", res["kernels_all_padding"])):
            for k, v in sorted(kk.items()):
                print(f"  [{name}] {k[:60]:60s} x{v['calls_per_batch']:.1f}  median {v['median_us']:9.1f} us  (min {v['min_us']:.1f}, max {v['max_us']:.1f})")
        print(json.dumps(res))
        return

    calls = []
    real = lib.call
    lib.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    call()
    lib.call = real
    res["abi_calls_per_batch"] = calls
    rates = []
    for _ in range(args.rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):
            call()
        b.record()
        torch.cuda.synchronize()
        rates.append(B * args.calls / (a.elapsed_time(b) * 1e-3))
    res["device_images_per_s"] = {"median": statistics.median(rates), "min": min(rates), "max": max(rates), "rounds": args.rounds,
                                  "calls_per_round": args.calls}
    print(f"device: {statistics.median(rates):.0f} images/s (min {min(rates):.0f}, max {max(rates):.0f} over {args.rounds} rounds of {args.calls} calls)")
    if not args.no_host:
        torch.set_num_threads(1)
        ref = host_worker(host, sizes, flips, pad)
        got = call().tensors.cpu()
        res["device_equals_host_worker"] = bool(torch.equal(got, ref))
        hr = []
        for _ in range(3):
            t0 = time.perf_counter()
            host_worker(host, sizes, flips, pad)
            hr.append(B / (time.perf_counter() - t0))
        res["host_worker_images_per_s"] = {"median": statistics.median(hr), "min": min(hr), "max": max(hr), "rounds": 3, "threads": 1}
        print(f"host worker (PIL + torch, 1 thread): {statistics.median(hr):.1f} images/s (min {min(hr):.1f}, max {max(hr):.1f}); "
              f"device result equals it bit for bit: {res['device_equals_host_worker']}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
