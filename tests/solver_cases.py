"""Case table of the grounding solver kernels (csrc/solver.hip): fiber_grad_sqnorm_multi_f32, fiber_solver_finalize and
fiber_adamw_torch_multi_f32 with hand-built tables, the fp64 restatement of one step and its per-element bounds.  Shared by
tests/test_hip_solver.py and tests/test_solver_host.py.  Importing it needs no GPU.

One step, in fp64 from the fp32 state, the fp32 scalars the kernel receives (b1, b2, eps, d, max_norm, {lr, wd} rows) and -- on the GPU -- the
clip coefficient c and the coefficient rows {decay, s1, r2} the finalize kernel STORED:
  norm = sqrt(sum g^2)        c = min(1, max_norm / (norm + 1e-6))        (a non-finite sum: c = 0, skip = 1, nothing but the EMA moves)
  decay = 1 - lr wd           s1 = lr / (1 - b1^t)                        r2 = 1 / sqrt(1 - b2^t)             t = the tensor's count + 1
  g' = c g       m' = b1 m + (1 - b1) g'       v' = b2 v + (1 - b2) g' g'              (1 - b1, 1 - b2, 1 - d formed in fp32)
  p1 = p decay   p' = p1 - s1 m' / (sqrt(v') r2 + eps)      ema' = d ema + (1 - d) p'
Bounds, |got - ref| <= K 2^-24 term + 2^-147 (fp32 denormal results: 2^-150 an operation), K = 2 x the number of rounded fp32 operations
on the path (the compiler may contract to FMA, which only removes roundings: K is a ceiling):
  M    c g, (1 - b1) g', b1 m, the sum                                         4 operations, K = 8    term |b1 m| + |(1 - b1) g'|
  V    c g, g' g', (1 - b2) (.), b2 v, the sum                                 5 operations, K = 10   term |b2 v| + |(1 - b2) g' g'|
  P    p decay, sqrt, r2 (.), + eps, s1 m', the quotient, the difference       7 operations, K = 14   term |p1| + |update|
       -- the reference taken from the m', v' the kernel stored (what it divides by)
  EMA  d ema, (1 - d) p', the sum                                              3 operations, K = 6    term |d ema| + |(1 - d) p'|
       -- from the p' the kernel stored
These K are derived from the arithmetic, not calibrated.  The bf16 working copy equals bf16(p') of the stored p' to the bit.
Scalars: norm, c and every coefficient are one rounding from fp64, so each lies within 2 x 2^-24 relative of its fp64 value (the fp64
summation error, at most N 2^-53 relative, is far below that); the device step counts are exact."""
import math

import numpy as np
import torch

from tests import optim_cases as oc
from tests.optim_cases import F32, TINY32, CHUNK, GUARD, SENTINEL, _view, bf16_bits  # noqa: F401

K = {"M": 8.0, "V": 10.0, "P": 14.0, "EMA": 6.0}
SCALAR_REL = 2.0 * F32
COLS = 7
BIG = 300 * CHUNK + 5                        # more than 256 partials for the finalize kernel to sum
N_SMALL = 300                                # ... and more than 256 tensors for its per-tensor loop
EMA_DECAY = 0.999

# (numel, gradient bytes past 16-byte alignment, p / m / v bytes into their allocation, bf16 copy: None | bytes, ema bytes into its allocation)
TENSORS = [t + (t[2],) for t in oc.TENSORS]
TENSORS[4] = TENSORS[4][:4] + (8,)           # n = 4095: the EMA alone off its alignment
TENSORS.append((BIG, 0, 0, 0, 0))
TENSORS += [(1 + i % 7, 4 * (i % 4), 0, None if i % 2 else 0, 0) for i in range(N_SMALL)]
INF_AT = (8, 7)                              # (tensor, element) of the inf gradient of the `inf` case


def _mixed(i):
    """per-tensor {lr, wd}: four learning rates, three decays (one of them 0)"""
    return (1e-4, 1e-3, 2e-5, 5e-4)[i % 4], (0.05, 0.0, 0.0125)[i % 3]


# max_norm: None = clipping off (the host passes +inf).  The gradient norm of every case is ~1e16 (one 1e15 element in each tensor of five
# elements or more), so 1e20 is well above it and 1e15 below it (c ~ 0.1).
CASES = [
    dict(name="step1_off_ema", step=1, hyper="uniform", lr=1e-4, wd=0.01, max_norm=None, ema="all"),
    dict(name="step1000_wd0_noema", step=1000, hyper="uniform", lr=3e-5, wd=0.0, max_norm=None, ema="none"),
    dict(name="mixed_above_some", step=1000, hyper="mixed", max_norm=1e20, ema="some"),
    dict(name="mixed_below_ema", step=1, hyper="mixed", max_norm=1e15, ema="all"),
    dict(name="inf_some", step=1000, hyper="mixed", max_norm=1e15, ema="some", inf=True),
]
for _c in CASES:
    _c.update(b1=0.9, b2=0.999, eps=1e-8, d=EMA_DECAY)
BY_NAME = {c["name"]: c for c in CASES}


def f32(x):
    return float(np.float32(x))


def has_ema(case, i):
    return case["ema"] == "all" or (case["ema"] == "some" and i % 3 != 1)


def hyper_rows(case):
    """float32 [n, 2] = {lr, wd} per tensor"""
    rows = [_mixed(i) if case["hyper"] == "mixed" else (case["lr"], case["wd"]) for i in range(len(TENSORS))]
    return np.array(rows, dtype=np.float32)


def prior_steps(case):
    """the counts before the step: step - 1 everywhere, or (mixed) up to two more, so that tensors of one launch differ"""
    return np.array([case["step"] - 1 + (i % 3 if case["hyper"] == "mixed" else 0) for i in range(len(TENSORS))], dtype=np.int32)


def chunk_table():
    """(tensor, chunk) pairs: tensors in reverse order, the chunks of tensors 7 and 8 interleaved as in optim_cases"""
    per = {i: [(i, c) for c in range(-(-t[0] // CHUNK))] for i, t in enumerate(TENSORS)}
    inter = [p for pair in zip(per[7], per[8]) for p in pair]
    rest = [p for i in reversed(range(len(TENSORS))) if i not in (7, 8) for p in per[i]]
    return rest[:5] + inter + rest[5:]


_state_cache = {}


def make_state(case):
    """per tensor: p, g, m, v, ema float32 numpy (read-only, shared between tests).  Gradients hold 0 (with m = v = 0), 1e-20 and 1e15
    where the tensor has five elements or more (optim_cases' specials); there p[3] = ema[3] = 0 as well, a zero-initialised parameter
    with a tiny gradient, whose update is not hidden behind |p|.  The `inf` case has one inf gradient element."""
    key = bool(case.get("inf"))
    if key in _state_cache:
        return _state_cache[key]
    g_ = torch.Generator().manual_seed(1234)
    out = []
    for i, (n, *_r) in enumerate(TENSORS):
        p = torch.randn(n, generator=g_).numpy()
        g = (torch.randn(n, generator=g_) * 0.02).numpy()
        m = (torch.randn(n, generator=g_) * 0.01).numpy()
        v = (torch.randn(n, generator=g_) * 0.01).numpy() ** 2
        e = torch.randn(n, generator=g_).numpy()
        if n >= 5:
            g[1], m[1], v[1] = 0.0, 0.0, 0.0
            g[2], g[n - 1] = 1e-20, 1e15
            g[3], m[3], v[3], p[3], e[3] = 1e-20, 0.0, 0.0, 0.0, 0.0
        if key and i == INF_AT[0]:
            g[INF_AT[1]] = np.inf
        d = {k: a.astype(np.float32) for k, a in dict(p=p, g=g, m=m, v=v, ema=e).items()}
        for a in d.values():
            a.setflags(write=False)
        out.append(d)
    _state_cache[key] = out
    return out


# ---- the fp64 restatement --------------------------------------------------------------------------------------------------------------------
def scalars_reference(case, state):
    """-> (norm, c, skip) in fp64 from the fp32 gradients and the fp32 max_norm"""
    total = math.fsum(float(np.sum(st["g"].astype(np.float64) ** 2)) for st in state)
    if not math.isfinite(total):
        return math.sqrt(total) if total == math.inf else math.nan, 0.0, 1
    norm = math.sqrt(total)
    mx = math.inf if case["max_norm"] is None else f32(case["max_norm"])
    return norm, min(1.0, mx / (norm + 1e-6)), 0


def coef_reference(case, steps_after):
    """fp64 [n, 3] = {decay, s1, r2} for the counts AFTER the step"""
    h = hyper_rows(case).astype(np.float64)
    t = steps_after.astype(np.float64)
    b1, b2 = f32(case["b1"]), f32(case["b2"])
    return np.stack([1.0 - h[:, 0] * h[:, 1], h[:, 0] / (1.0 - b1 ** t), 1.0 / np.sqrt(1.0 - b2 ** t)], axis=1)


def moments_reference(case, st, c, mutate=None):
    """-> m', v' (fp64) and their bound terms; c: the clip coefficient (fp64 value of what the kernel used)"""
    b1, b2 = np.float32(case["b1"]), np.float32(case["b2"])
    omb1, omb2 = float(np.float32(1) - b1), float(np.float32(1) - b2)
    g, m, v = (st[k].astype(np.float64) for k in ("g", "m", "v"))
    g1 = c * g
    gv = g if mutate == "c_m_only" else g1
    m1, v1 = float(b1) * m + omb1 * g1, float(b2) * v + omb2 * gv * gv
    return m1, v1, np.abs(float(b1) * m) + np.abs(omb1 * g1), np.abs(float(b2) * v) + np.abs(omb2 * g1 * g1)


def param_reference(case, p, m1, v1, row, mutate=None):
    """p' (fp64) from the moments given (the kernel's stored ones on the GPU, the reference's on the host) and the coefficient row
    {decay, s1, r2}; and its bound term"""
    decay, s1, r2 = (float(x) for x in row[:3])
    eps = f32(case["eps"])
    p = p.astype(np.float64)
    den = (np.sqrt(v1) + eps) * r2 if mutate == "eps_before" else np.sqrt(v1) * r2 + eps
    upd = s1 * m1 / den
    if mutate == "decay_after":
        return (p - upd) * decay, np.abs(p * decay) + np.abs(upd)
    return p * decay - upd, np.abs(p * decay) + np.abs(upd)


def ema_reference(case, ema, p_new):
    """ema' (fp64) from the parameter given (the stored p', or the unchanged p of a skipped step) and its bound term"""
    d = np.float32(case["d"])
    omd = float(np.float32(1) - d)
    a, b = float(d) * ema.astype(np.float64), omd * np.asarray(p_new, dtype=np.float64)
    return a + b, np.abs(a) + np.abs(b)


def reference_step(case, state, steps_before=None, mutate=None):
    """The whole step in fp64 -> an `out` dict of the layout run_step() returns (numpy fp64 instead of fp32): what a kernel without
    rounding would leave.  mutate: "decay_after" (decay applied to the updated parameter), "eps_before" (eps added before the division
    by sqrt(1 - b2^t)), "c_m_only" (the clip coefficient applied to m' but not v'), "ema_from_p" (the EMA taken from p instead of p')."""
    steps_before = prior_steps(case) if steps_before is None else steps_before
    norm, c, skip = scalars_reference(case, state)
    out = dict(norm=norm, c=c, skip=skip, skipped=skip, steps=steps_before + (0 if skip else 1), tensors=[])
    out["coef"] = None if skip else coef_reference(case, out["steps"])
    for i, st in enumerate(state):
        if skip:
            d = dict(p=st["p"].astype(np.float64), m=st["m"].astype(np.float64), v=st["v"].astype(np.float64))
        else:
            m1, v1, _, _ = moments_reference(case, st, c, mutate)
            p1, _ = param_reference(case, st["p"], m1, v1, out["coef"][i], mutate)
            d = dict(p=p1, m=m1, v=v1)
        if has_ema(case, i):
            d["ema"] = ema_reference(case, st["ema"], st["p"] if mutate == "ema_from_p" else d["p"])[0]
        out["tensors"].append(d)
    return out


def verify_step(case, state, out, steps_before=None, check=None, record=None):
    """Every check of one step on `out` (run_step()'s layout) against the restatement.  check(name, got, ref, bound) asserts per element
    (default: hip_util.assert_elementwise) and returns the worst |err| / bound; record(kind, ratio) is told each worst ratio with K = 1."""
    from tests.hip_util import assert_elementwise
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).reshape(-1, 1)   # noqa: E731
    check = check or (lambda name, got, ref, bound: assert_elementwise(name, T(got), T(ref), T(bound)))
    steps_before = prior_steps(case) if steps_before is None else steps_before
    norm, c, skip = scalars_reference(case, state)
    assert out["skip"] == skip, f"{case['name']}: skip {out['skip']}, expected {skip}"
    if skip:
        assert out["c"] == 0.0 and not math.isfinite(out["norm"])
        assert np.array_equal(out["steps"], steps_before), "a skipped step advanced a count"
    else:
        assert abs(out["norm"] - norm) <= SCALAR_REL * norm, (out["norm"], norm)
        assert abs(out["c"] - c) <= SCALAR_REL * c, (out["c"], c)
        assert np.array_equal(out["steps"], steps_before + 1), "step counts"
        cref = coef_reference(case, steps_before + 1)
        got = np.asarray(out["coef"], dtype=np.float64)[:, :3]
        bad = np.abs(got - cref) > SCALAR_REL * np.abs(cref)
        assert not bad.any(), f"{case['name']}: coefficient rows {np.argwhere(bad)[:4].tolist()}: {got[bad][:4]} vs {cref[bad][:4]}"
    for i, (st, d) in enumerate(zip(state, out["tensors"])):
        tag = f"{case['name']} tensor {i} (n = {st['p'].size})"
        if skip:
            for k in ("p", "m", "v"):
                assert np.array_equal(np.asarray(d[k], dtype=np.float64), st[k].astype(np.float64)), f"{tag}: a skipped step changed {k}"
        else:
            m1, v1, tm, tv = moments_reference(case, st, float(out["c"]))
            p1, tp = param_reference(case, st["p"], np.asarray(d["m"], np.float64), np.asarray(d["v"], np.float64), np.asarray(out["coef"])[i])
            for kind, got, ref, term in (("M", d["m"], m1, tm), ("V", d["v"], v1, tv), ("P", d["p"], p1, tp)):
                r = check(f"{tag} {kind}", got, ref, K[kind] * F32 * term + TINY32)
                if record:
                    record(kind, r * K[kind])
        assert ("ema" in d) == has_ema(case, i)
        if "ema" in d:
            e1, te = ema_reference(case, st["ema"], np.asarray(d["p"], np.float64))
            r = check(f"{tag} EMA", d["ema"], e1, K["EMA"] * F32 * te + TINY32)
            if record:
                record("EMA", r * K["EMA"])


# ---- the runner ------------------------------------------------------------------------------------------------------------------------------
def build(case, state, device="cuda", steps_before=None):
    """Device buffers (views with SENTINEL guards), tables and the state block of one case -> ctx"""
    bufs = []
    dev = lambda a: torch.tensor(a).to(device)          # noqa: E731  (a copy: the shared state is read-only)
    for i, ((n, goff, poff, woff, eoff), st) in enumerate(zip(TENSORS, state)):
        d = {}
        for k in ("p", "m", "v"):
            d[k + "_buf"], d[k] = _view(n, poff, torch.float32, dev(st[k]), device)
        d["g_buf"], d["g"] = _view(n, goff, torch.float32, dev(st["g"]), device)
        if woff is not None:
            d["w_buf"], d["w"] = _view(n, woff, torch.bfloat16, None, device)
        if has_ema(case, i):
            d["ema_buf"], d["ema"] = _view(n, eoff, torch.float32, dev(st["ema"]), device)
        assert d["g"].data_ptr() % 16 == goff and d["p"].data_ptr() % 16 == poff
        bufs.append(d)
    n = len(TENSORS)
    chunks = chunk_table()
    steps_before = prior_steps(case) if steps_before is None else steps_before
    ctx = dict(bufs=bufs, n=n, nchunks=len(chunks))
    ctx["coef"] = torch.full((n + GUARD, 4), SENTINEL, dtype=torch.float32, device=device)
    ctx["steps"] = torch.cat([torch.from_numpy(steps_before), torch.full((GUARD,), -77, dtype=torch.int32)]).to(device)
    ctx["partial"] = torch.full((len(chunks) + GUARD,), SENTINEL, dtype=torch.float64, device=device)
    ctx["block"] = torch.tensor([0, 0, 0, 0] + [-77] * GUARD, dtype=torch.int32).to(device)
    ctx["lr_wd"] = torch.from_numpy(hyper_rows(case)).to(device)
    ptr = lambda d, k: d[k].data_ptr() if k in d else 0     # noqa: E731
    ctx["table"] = torch.tensor([[ptr(d, "p"), ptr(d, "g"), ptr(d, "m"), ptr(d, "v"), ptr(d, "w"), ptr(d, "ema"), ctx["coef"].data_ptr() + 16 * i]
                                 for i, d in enumerate(bufs)], dtype=torch.int64).to(device)
    ctx["numel"] = torch.tensor([t[0] for t in TENSORS], dtype=torch.int64).to(device)
    ctx["chunks"] = torch.tensor(chunks, dtype=torch.int32).to(device)
    return ctx


def launch(lib, case, ctx):
    """the three entry points once over ctx -> `out`: scalars, counts, coefficient rows and per tensor p, m, v, (w), (ema) as numpy"""
    P = lib.ptr
    mx = float("inf") if case["max_norm"] is None else f32(case["max_norm"])
    lib.call("fiber_grad_sqnorm_multi_f32", P(ctx["table"]), P(ctx["numel"]), P(ctx["chunks"]), ctx["nchunks"], P(ctx["partial"]))
    lib.call("fiber_solver_finalize", P(ctx["partial"]), ctx["nchunks"], mx, P(ctx["lr_wd"]), P(ctx["steps"]), P(ctx["coef"]), ctx["n"],
             f32(case["b1"]), f32(case["b2"]), P(ctx["block"]))
    lib.call("fiber_adamw_torch_multi_f32", P(ctx["table"]), P(ctx["numel"]), P(ctx["chunks"]), ctx["nchunks"], f32(case["b1"]), f32(case["b2"]),
             f32(case["eps"]), f32(case["d"]), P(ctx["block"]))
    torch.cuda.synchronize()
    return read(ctx)


def read(ctx):
    n = ctx["n"]
    block = ctx["block"].cpu()
    out = dict(norm=float(block[0:1].view(torch.float32)[0]), c=float(block[1:2].view(torch.float32)[0]), skip=int(block[2]), skipped=int(block[3]),
               steps=ctx["steps"][:n].cpu().numpy(), coef=ctx["coef"][:n].cpu().numpy(), partial=ctx["partial"][:ctx["nchunks"]].cpu().numpy(),
               tensors=[])
    for d in ctx["bufs"]:
        t = {k: d[k].cpu().numpy() for k in ("p", "m", "v", "g", "ema") if k in d}
        if "w" in d:
            t["w"] = d["w"].view(torch.int16).cpu().numpy()
        out["tensors"].append(t)
    return out


def guards_untouched(ctx):
    """-> list of what was written outside its tensor (empty: nothing)"""
    bad = []
    for i, d in enumerate(ctx["bufs"]):
        for k in ("p", "m", "v", "g", "w", "ema"):
            if k in d:
                buf, view = d[k + "_buf"], d[k]
                lead = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
                rest = torch.cat([buf[:lead], buf[lead + view.numel():]])
                if not bool((rest == SENTINEL).all()):
                    bad.append((i, k))
    n = ctx["n"]
    if not bool((ctx["coef"][n:] == SENTINEL).all()):
        bad.append("coef")
    if not bool((ctx["steps"][n:] == -77).all()):
        bad.append("steps")
    if not bool((ctx["partial"][ctx["nchunks"]:] == SENTINEL).all()):
        bad.append("partial")
    if not bool((ctx["block"][4:] == -77).all()):
        bad.append("block")
    return bad
