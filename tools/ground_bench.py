"""Grounding head (csrc/ground.hip) timings at the detection geometry: 22 400 anchors (five levels of an 800 x 1344 input) x 256 tokens.
   python tools/ground_bench.py [out.md]
Per batch size 1, 2, 4: the fused token loss forward + backward (ops.ground_token_loss), the logits forward (ops.ground_logits) and the
plain-torch-on-device statement of the reference lines (vldyhead.py:857-891 + sigmoid_focal_loss.py:130-171, forward + backward) -- the
baseline: there was no earlier path.  Reported: microseconds (median of 20 after 5 warm-up calls), the algorithmic minimum of HBM bytes
(X + P + targets in, ds out) over the time, and the peak memory above the inputs."""
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fiber_amd import lib, ops

A, T, C = 22400, 256, 256


def timeit(fn, reps=20, warm=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    lib.load()
    lines = ["| B | fused loss fwd+bwd us | GB/s of the minimum | peak MiB | logits fwd us | peak MiB | torch fwd+bwd us | peak MiB |", "|---|---|---|---|---|---|---|---|"]
    for B in (1, 2, 4):
        x = torch.randn(B, A, C, device="cuda").to(torch.bfloat16).requires_grad_()
        p = (torch.randn(B, T, C, device="cuda") * 0.25).requires_grad_()
        tb = (torch.randn(B, T, device="cuda") - 2.0).requires_grad_()
        ls = torch.tensor([0.3], device="cuda", requires_grad=True)
        tg = (torch.rand(B, A, T, device="cuda") < 0.01).to(torch.uint8)
        mask = torch.ones(B, T, dtype=torch.uint8, device="cuda")

        def fused():
            ops.ground_token_loss(x, p, tb, ls, tg, mask, 0.25, 2.0).backward()

        def logits():
            with torch.no_grad():
                return ops.ground_logits(x, p, tb, ls)

        def plain():
            s = (torch.matmul(x.float(), p.transpose(-1, -2)) / ls.exp() + tb.unsqueeze(1).repeat(1, A, 1)).clamp(max=50000).clamp(min=-50000)
            m = (mask > 0).unsqueeze(1).repeat(1, A, 1)
            lg, t = torch.masked_select(s, m), torch.masked_select(tg.float(), m)
            pr = torch.sigmoid(lg)
            ce = torch.nn.functional.binary_cross_entropy_with_logits(lg, t, reduction="none")
            p_t = pr * t + (1 - pr) * (1 - t)
            ((0.25 * t + 0.75 * (1 - t)) * (ce * ((1 - p_t) ** 2.0))).sum().backward()

        minimum = B * (A * C * 2 + T * C * 2 + A * T + A * T * 2)       # X + P + targets in, ds out
        tf, tl, tp = timeit(fused), timeit(logits), timeit(plain)
        lines.append(f"| {B} | {tf:.0f} | {minimum / tf / 1e3:.0f} | {peak(fused):.0f} | {tl:.0f} | {peak(logits):.0f} | {tp:.0f} | {peak(plain):.0f} |")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
