"""s_memtime trace of the q8 GEMM's K loop (TRACE build, act bit FIBER_ACT_TRACE): cycles per K tile spent in each phase's load half /
wait+barrier / MFMA issue / barrier, for the first 8 workgroups x 8 waves.    python tools/gemm_trace.py q8"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fiber_amd import lib
lib.load()

def q8(M, N, K, act=0):
    """Per-wave, per-phase totals of the q8 kernel (TRACE build, act bit FIBER_ACT_TRACE): cycles per K tile."""
    x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    w = (torch.randn(N, K, device="cuda") * K ** -0.5).to(torch.bfloat16)
    b = torch.randn(N, device="cuda")
    y = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    pre = torch.empty(M, N, device="cuda", dtype=torch.bfloat16) if act == 1 else None
    dbg = torch.zeros(8 * 8 * 24, device="cuda")
    for _ in range(int(os.environ.get("FIBER_TRACE_LAUNCHES", "3"))):     # (a clock reading wants >= 2 s of back-to-back launches)
        lib.call("fiber_gemm_nt_bf16", lib.ptr(x), lib.ptr(w), lib.ptr(b), None, lib.ptr(y), lib.ptr(pre), None, 0, None, 0, lib.ptr(dbg),
                 M, N, K, K, K, N, 0, lib.DEFINES["FIBER_ACT_TRACE"] | act)
    torch.cuda.synchronize()
    d = dbg.view(8, 8, 24).cpu()
    nk, T = d[0, 0, 18].item(), d[0, 0, 19].item()
    print(f"q8 M={M} N={N} K={K} act={act}: nk={nk:.0f} tiles/wg={T:.0f}  (s_memtime ticks per K TILE; per phase: load half incl. read return / wait+barrier / MFMA issue / barrier)")
    for wg in (0, 5):
        for wv in (0, 3, 4, 7):
            r = d[wg, wv] / (T * nk)
            ph = " | ".join(f"P{p + 1} {r[4 * p]:5.0f} {r[4 * p + 1]:5.0f} {r[4 * p + 2]:5.0f} {r[4 * p + 3]:5.0f}" for p in range(4))
            print(f"wg{wg} wave{wv} g{wv // 4}: {ph} | epilogue/tile {d[wg, wv, 16] / T:7.0f} | total/Ktile {d[wg, wv, 17] / (T * nk):6.0f}")
    clk = (d[:, :, 20] / d[:, :, 21].clamp_min(1)).flatten() * 0.1     # s_memtime ticks per 100-MHz s_memrealtime tick over the K loops -> GHz
    print(f"in-kernel clock over the K loops: median {clk.median():.3f} GHz (min {clk.min():.3f}, max {clk.max():.3f}; 64 waves)")


if len(sys.argv) > 2:                                       # python tools/gemm_trace.py q8 M,N,K [M,N,K ...]
    for arg in sys.argv[2:]:
        q8(*(int(v) for v in arg.split(",")), 0)
else:
    for shp in ((294912, 2048, 512), (294912, 512, 2048), (73728, 1024, 4096)):
        q8(*shp, 0)
    q8(294912, 2048, 512, 1)
