"""GPU time of one grounding solver step on a Swin-B + RoBERTa-base + FPN + 6-conv DyHead sized parameter list (random tensors of those
shapes, one parameter group each):
  (a) optim.FiberTorchAdamW with clipping and the attached ModelEma: three launches of csrc/solver.hip (+ the cache refresh launches)
  (b) what the reference runs on the same tensors: clip_grad_norm_ + torch.optim.AdamW(foreach=True) + the per-entry EMA loop
and each of the three kernels alone against its traffic.  Warm-up, then the median of --reps repetitions, each between two events on the
stream.  --profile-launches counts the kernel launches of one step of each path with torch.profiler instead of timing (a run of its own).

    python tools/solver_bench.py [--reps 30] [--profile-launches]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from fiber_amd import lib, ops  # noqa: E402
from fiber_amd.optim import FiberTorchAdamW  # noqa: E402
from fiber_amd.solver import ModelEma  # noqa: E402

HBM_PEAK = 8.0e12     # bytes/s (MI355X_MICROARCH.md)
DEV = "cuda"


def shapes():
    out = [(128, 3, 4, 4), (128,), (128,), (128,)]                       # Swin-B: EMBED_DIM 128, DEPTHS (2, 2, 18, 2), window 12
    for stage, (depth, heads) in enumerate(zip((2, 2, 18, 2), (4, 8, 16, 32))):
        C = 128 << stage
        for _ in range(depth):
            out += [(C,), (C,), (3 * C, C), (3 * C,), (23 * 23, heads), (C, C), (C,), (C,), (C,), (4 * C, C), (4 * C,), (C, 4 * C), (C,)]
        if stage < 3:
            out += [(4 * C,), (4 * C,), (2 * C, 4 * C)]
    out += [(1024,), (1024,)]
    out += [(50265, 768), (514, 768), (1, 768), (768,), (768,)]         # RoBERTa-base
    for _ in range(12):
        out += [(768, 768), (768,)] * 4 + [(768,), (768,), (3072, 768), (3072,), (768, 3072), (768,), (768,), (768,)]
    out += [(256, c, 1, 1) for c in (256, 512, 1024)] + [(256,)] * 3 + [(256, 256, 3, 3)] * 5 + [(256,)] * 5      # FPN + P6 / P7
    for _ in range(6):                                                   # DyHead: three deformable 3x3, their norms, offsets, attention, DyReLU
        out += [(256, 256, 3, 3)] * 3 + [(256,)] * 6 + [(27, 256, 3, 3), (27,), (1, 256, 1, 1), (1,), (64, 256), (64,), (1024, 64), (1024,)]
    out += [(4, 256, 1, 1), (4,), (1, 256, 1, 1), (1,), (256, 768), (256,), (768, 256), (768,)]                        # the heads
    return out


class Params(torch.nn.Module):
    def __init__(self, shp, seed):
        super().__init__()
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.p = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, device=DEV, generator=g) * 0.02) for s in shp])


def set_grads(model, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    for p in model.p:
        p.grad = torch.randn(p.shape, device=DEV, generator=g) * 1e-3


def groups(model):
    return [{"params": [p], "lr": 1e-4 if i % 2 else 5e-5, "weight_decay": 0.05 if p.dim() > 1 else 0.0} for i, p in enumerate(model.p)]


def median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = [a.elapsed_time(b) for a, b in ev]
    return statistics.median(t), min(t), max(t)


def reference_ema_update(ema_model, model, d):
    """the per-entry loop of the reference's utils/ema.py:36-45, restated"""
    with torch.no_grad():
        src = model.state_dict()
        for k, e in ema_model.state_dict().items():
            e.copy_(e * d + (1.0 - d) * src[k].detach())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--profile-launches", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "solver_bench needs a HIP device"
    lib.load()
    shp = shapes()
    numel = sum(int(torch.Size(s).numel()) for s in shp)
    d = 0.999

    # (a)
    ma = Params(shp, 1)
    for p in ma.p:
        if p.dim() == 2:
            ops.bf16_weight(p)                                            # the GEMM weights have a cached bf16 working copy in training
    ema_a = ModelEma(ma, d)
    opt_a = FiberTorchAdamW(groups(ma), lr=1e-4, max_grad_norm=1.0)
    opt_a.attach_ema(ema_a)
    set_grads(ma, 2)
    calls = []
    real_call = lib.call

    def counting_call(name, *a):
        calls.append(name)
        return real_call(name, *a)

    def step_a():
        opt_a.step()
        ema_a.update(ma)

    # (b)
    mb = Params(shp, 1)
    ema_b = ModelEma(mb, d).ema
    opt_b = torch.optim.AdamW(groups(mb), lr=1e-4, foreach=True)
    set_grads(mb, 2)
    all_b = list(mb.p)

    def step_b():
        torch.nn.utils.clip_grad_norm_(all_b, 1.0)
        opt_b.step()
        reference_ema_update(ema_b, mb, d)

    if args.profile_launches:
        from torch.profiler import ProfilerActivity, profile
        counts = {}
        for name, fn in (("a", step_a), ("b", step_b)):
            fn()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            counts[name] = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                               and "memset" not in e.name.lower())
        print(json.dumps({"kernel_launches": counts}))
        return

    lib.call = counting_call
    ops.lib.call = counting_call
    step_a()
    calls.clear()
    step_a()
    launches_a = list(calls)
    lib.call = real_call
    ops.lib.call = real_call
    ta = median_ms(step_a, args.reps)
    tb = median_ms(step_b, args.reps)

    # the kernels alone, on the tables of (a)
    tab, P = opt_a._tab, lib.ptr
    block = opt_a._state_block()
    n_copy = sum(p.numel() for p in ma.p if ops.bf16_copy_if_cached(p) is not None)
    bytes_norm = 4 * numel + 8 * tab["nchunks"]
    bytes_fin = 8 * tab["nchunks"] + tab["n"] * (8 + 8 + 16)
    bytes_adam = (16 + 12 + 8) * numel + 2 * n_copy
    k_norm = median_ms(lambda: lib.call("fiber_grad_sqnorm_multi_f32", P(tab["table"]), P(tab["numel"]), P(tab["chunks"]), tab["nchunks"],
                                        P(tab["partial"])), args.reps)
    k_fin = median_ms(lambda: lib.call("fiber_solver_finalize", P(tab["partial"]), tab["nchunks"], 1.0, P(tab["lr_wd"]), P(tab["steps"]),
                                       P(tab["coef"]), tab["n"], 0.9, 0.999, P(block)), args.reps)
    k_adam = median_ms(lambda: lib.call("fiber_adamw_torch_multi_f32", P(tab["table"]), P(tab["numel"]), P(tab["chunks"]), tab["nchunks"], 0.9,
                                        0.999, 1e-8, d, P(block)), args.reps)
    res = {"tensors": len(shp), "elements": numel, "chunks": tab["nchunks"], "reps": args.reps,
           "a_fiber_ms": {"median": ta[0], "min": ta[1], "max": ta[2]}, "b_torch_ms": {"median": tb[0], "min": tb[1], "max": tb[2]},
           "a_launches": len(launches_a), "a_launch_names": sorted(set(launches_a)),
           "kernels": {name: {"ms": t[0], "bytes": b, "bytes_per_s": b / (t[0] * 1e-3), "of_hbm_peak": b / (t[0] * 1e-3) / HBM_PEAK}
                       for name, t, b in (("grad_sqnorm", k_norm, bytes_norm), ("finalize", k_fin, bytes_fin), ("adamw_torch", k_adam, bytes_adam))}}
    print(f"{len(shp)} tensors, {numel / 1e6:.1f} M elements, {tab['nchunks']} chunks")
    print(f"(a) FiberTorchAdamW + EMA   median {ta[0]:.3f} ms (min {ta[1]:.3f}, max {ta[2]:.3f}), {len(launches_a)} launches: {sorted(set(launches_a))}")
    print(f"(b) clip + AdamW(foreach) + EMA loop   median {tb[0]:.3f} ms (min {tb[1]:.3f}, max {tb[2]:.3f})")
    for k, v in res["kernels"].items():
        print(f"    {k:12s} {v['ms'] * 1e3:9.1f} us  {v['bytes'] / 1e6:9.2f} MB  {v['bytes_per_s'] / 1e12:6.3f} TB/s  ({100 * v['of_hbm_peak']:.1f} % of 8 TB/s)")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
