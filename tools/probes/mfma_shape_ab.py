"""Same-process A/B of two builds of libfiber_hip.so on the shapes gemm_nt_q8_kernel and the 256-tile gemm_tn_kernel serve in the bench step.

    make -C fiber_amd/csrc OBJDIR=$PWD/.ab/objB OUT=$PWD/.ab/libfiber_hip_B.so EXTRA=-DSOME_VARIANT     (a second build beside the product's)
    python tools/probes/mfma_shape_ab.py --a fiber_amd/libfiber_hip.so --b .ab/libfiber_hip_B.so [--rounds 7] [--json out.json]

Both libraries are loaded into this process (ctypes.CDLL on two paths) and fiber_gemm_nt_bf16 / fiber_gemm_tn_bf16 / fiber_gemm_tn_rowmap_bf16
of each are timed with HIP events on the same randn operands (never zeros: the chip holds a higher clock on trivial data and the two MFMA
shapes then rank by cycles alone), interleaved per round and per shape, the order of the arms alternating from round to round.  The shapes
are the (entry, kind, shape) rows of profiles/r06_roofline_by_shape.md that the two kernels serve, each weighted by its calls per step.
Printed: median and min per arm and shape, the weighted ms per step of every round, and per kernel the difference of the medians against
three times arm A's own round-to-round spread (max - min of its per-round weighted sums).

    python tools/probes/mfma_shape_ab.py --a A_probe.so --b B_probe.so --clock
reads the in-kernel clock of the weight-gradient kernel instead (diagnostic only): both libraries built with EXTRA=-DFIBER_TN_CLOCK_PROBE stamp
s_memtime and s_memrealtime around each workgroup's K loop; after >= 2 s of back-to-back launches per arm the quotient x 100 MHz is the clock the
chip held, and the s_memtime difference alone the cycles.  (The q8 kernel's reading comes from its TRACE build: tools/gemm_trace.py.)"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from fiber_amd import lib as flib

BF = torch.bfloat16
BATCH = 256                                                  # samples of the bench step: rows per sample = M / BATCH


def table_rows(path):
    """(entry, kind, M, N, K, calls) of every GEMM row of the roofline table."""
    rows = []
    for ln in open(path):
        m = re.match(r"\| (gemm_nt|gemm_tn|gemm_tn_rowmap) \| ([^|]+) \| \[(\d+), (\d+), (\d+)\] \| (\d+) \|", ln)
        if m:
            rows.append((m.group(1), m.group(2).strip(), int(m.group(3)), int(m.group(4)), int(m.group(5)), int(m.group(6))))
    return rows


def served(entry, M, N, K):
    """Does the call reach gemm_nt_q8_kernel / the 256-tile gemm_tn_kernel?  (gemm_plan / tn_plan of the csrc files, default environment;
    every NT kind of the table is an epilogue q8 is built for.)"""
    if entry == "gemm_nt":
        tiles = -(-M // 256) * -(-N // 256)
        return tiles >= 200 and K >= 128 and K % 64 == 0 and (N % 256 == 0 or (N % 64 == 0 and N > 256))
    return N >= 192 and K >= 192


def load(path):
    lib = C.CDLL(os.path.abspath(path))
    for name in ("fiber_gemm_nt_bf16", "fiber_gemm_tn_bf16", "fiber_gemm_tn_rowmap_bf16"):
        fn = getattr(lib, name)
        fn.argtypes = flib.SIGNATURES[name] + [flib.P]
        fn.restype = flib.I
    lib.fiber_gemm_tn_splits.argtypes = [flib.I] * 3
    lib.fiber_gemm_tn_splits.restype = flib.I
    return lib


def ptr(t):
    return None if t is None else t.data_ptr()


def make_call(entry, kind, M, N, K, libs):
    """Operands of one row (shared by the arms) and call(lib)."""
    g = torch.Generator(device="cuda").manual_seed(M + 7 * N + 31 * K)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    rps = M // BATCH
    keep = (torch.rand(BATCH, device="cuda", generator=g) > 0.1).float() / 0.9
    if entry == "gemm_nt":
        x, w = rn(M, K).to(BF), (rn(N, K) * K ** -0.5).to(BF)
        bias = rn(N) * 0.5
        y = torch.empty(M, N, device="cuda", dtype=BF)
        res = rn(M, N).to(BF) if "residual" in kind else None
        rs = keep if "droppath" in kind else None
        act = 1 if "gelu+pre" in kind else 2 if "gelu'" in kind else 0
        pre = torch.empty_like(y) if act == 1 else None
        aux = (rn(M, N) * 1.5).to(BF) if act == 2 else None
        args = (ptr(x), ptr(w), None if act == 2 else ptr(bias), ptr(res), ptr(y), ptr(pre), ptr(rs), rps if rs is not None else 0, ptr(aux),
                N if aux is not None else 0, None, M, N, K, K, K, N, N if res is not None else 0, act)
        hold = (x, w, bias, y, res, rs, pre, aux)
        name = "fiber_gemm_nt_bf16"
    else:
        dy, x = rn(M, N).to(BF), rn(M, K).to(BF)
        dw, db = torch.empty(N, K, device="cuda"), torch.empty(N, device="cuda")
        S = {lb.fiber_gemm_tn_splits(M, N, K) for lb in libs}
        assert len(S) == 1, "the two builds split this problem differently"
        ws = torch.empty(S.pop() * (N * K + N), device="cuda")
        mask = keep if "droppath" in kind else None
        assert mask is None or rps % 64 == 0
        args = (ptr(dy), ptr(x), ptr(dw), ptr(db), ptr(ws), M, N, K, N, K, ptr(mask), rps if mask is not None else 0, 1 / 0.9 if mask is not None else 1.0)
        hold = (dy, x, dw, db, ws, mask)
        name = "fiber_gemm_tn_bf16"
        if entry == "gemm_tn_rowmap":
            perm = torch.randperm(N, device="cuda", generator=g).to(torch.int32)
            args, hold, name = args + (ptr(perm),), hold + (perm,), "fiber_gemm_tn_rowmap_bf16"

    def call(lb):
        rc = getattr(lb, name)(*args, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, (name, rc)
    return call, hold


def timed(call, lb, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call(lb)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


CLOCK_SHAPES = [("gemm_tn", "TN wgrad", 294912, 2048, 512), ("gemm_tn", "TN wgrad", 294912, 512, 2048), ("gemm_tn", "TN wgrad", 73728, 1024, 4096)]


def clock_mode(libs, seconds=2.0):
    for lb in libs.values():
        lb.fiber_gemm_tn_clock_probe.argtypes = [C.c_void_p, C.c_int]
        lb.fiber_gemm_tn_clock_probe.restype = C.c_int
    for entry, kind, M, N, K in CLOCK_SHAPES:
        call, hold = make_call(entry, kind, M, N, K, list(libs.values()))
        for arm in "ABAB":                                    # each arm twice, alternating
            lb = libs[arm]
            n = max(10, int(seconds * 1e3 / max(timed(call, lb, 5), 1e-3)))
            ms = timed(call, lb, n)
            buf = (C.c_ulonglong * 512)()
            assert lb.fiber_gemm_tn_clock_probe(buf, 256) == 0
            cyc = sorted(buf[2 * i] for i in range(256))
            ghz = sorted(0.1 * buf[2 * i] / max(buf[2 * i + 1], 1) for i in range(256))
            print(f"{arm} [{M}, {N}, {K}]: {ms:.4f} ms per call over {n} launches; K loop {cyc[128]} cycles (median of 256 workgroups), "
                  f"clock {ghz[128]:.3f} GHz (min {ghz[0]:.3f}, max {ghz[-1]:.3f})", flush=True)
        del call, hold
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", required=True, help="library of arm A (the reference arm: its spread sets the decision threshold)")
    ap.add_argument("--b", required=True)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--table", default=os.path.join(ROOT, "profiles", "r06_roofline_by_shape.md"))
    ap.add_argument("--target-ms", type=float, default=40.0, help="back-to-back launches per measurement add up to about this long")
    ap.add_argument("--json", default=None)
    ap.add_argument("--clock", action="store_true", help="in-kernel clock of the TN kernel (both libraries built with -DFIBER_TN_CLOCK_PROBE)")
    a = ap.parse_args()
    assert a.rounds >= 5
    torch.cuda.set_device(0)
    libs = {"A": load(a.a), "B": load(a.b)}
    if a.clock:
        print(f"A = {a.a}\nB = {a.b}")
        return clock_mode(libs)
    rows = [r for r in table_rows(a.table) if served(r[0], *r[2:5])]
    print(f"A = {a.a}\nB = {a.b}\n{len(rows)} rows, {a.rounds} rounds\n| entry | kind | shape | calls | A median ms | A min | B median ms | B min | B / A | A TFLOP/s |\n"
          "|---|---|---|---|---|---|---|---|---|---|", flush=True)
    per = {}                                                  # row -> arm -> [ms per call, one per round]
    for r in rows:
        entry, kind, M, N, K, calls = r
        call, hold = make_call(entry, kind, M, N, K, list(libs.values()))
        for arm in "AB":                                      # warm-up: code objects loaded, caches and clocks settled
            timed(call, libs[arm], 3)
        reps = max(3, int(a.target_ms / max(timed(call, libs["A"], 3), 1e-3)))
        per[r] = {"A": [], "B": []}
        for rd in range(-1, a.rounds):                        # round -1 is a warm-up at full length and is discarded: the first full-length round of
            for arm in ("AB" if rd % 2 == 0 else "BA"):       # a shape read 1-3 % high in BOTH arms (clock and caches still settling)
                t = timed(call, libs[arm], reps)
                if rd >= 0:
                    per[r][arm].append(t)
        md = {arm: statistics.median(per[r][arm]) for arm in "AB"}
        mn = {arm: min(per[r][arm]) for arm in "AB"}
        tf = 2.0 * M * N * K / md["A"] * 1e-9
        print(f"| {entry} | {kind} | [{M}, {N}, {K}] | {calls} | {md['A']:.4f} | {mn['A']:.4f} | {md['B']:.4f} | {mn['B']:.4f} | {md['B'] / md['A']:.4f} | {tf:.0f} |", flush=True)
        del call, hold
        torch.cuda.empty_cache()
    out = {"a": a.a, "b": a.b, "rows": [dict(entry=r[0], kind=r[1], shape=r[2:5], calls=r[5], **per[r]) for r in rows], "kernels": {}}
    for kern, pick in (("gemm_nt_q8_kernel", lambda r: r[0] == "gemm_nt"), ("gemm_tn_kernel<256>", lambda r: r[0] != "gemm_nt")):
        sums = {arm: [sum(r[5] * per[r][arm][rd] for r in rows if pick(r)) for rd in range(a.rounds)] for arm in "AB"}
        med = {arm: statistics.median(sums[arm]) for arm in "AB"}
        spread = max(sums["A"]) - min(sums["A"])
        gain = med["A"] - med["B"]
        print(f"\n{kern}: weighted ms per step, per round\n  A {' '.join(f'{v:.3f}' for v in sums['A'])}   median {med['A']:.3f}  min {min(sums['A']):.3f}"
              f"\n  B {' '.join(f'{v:.3f}' for v in sums['B'])}   median {med['B']:.3f}  min {min(sums['B']):.3f}"
              f"\n  A - B = {gain:+.3f} ms ({100 * gain / med['A']:+.2f} %), spread of A {spread:.3f} ms, threshold 3 x spread = {3 * spread:.3f} ms"
              f" -> B {'WINS' if gain > 3 * spread else 'does not win'}")
        out["kernels"][kern] = dict(sums=sums, median=med, spread_a=spread, gain_ms=gain, b_wins=gain > 3 * spread)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"))


if __name__ == "__main__":
    main()
