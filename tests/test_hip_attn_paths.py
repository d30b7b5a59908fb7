"""Every attention kernel path, element by element against fp64 (tests/attn_cases.py: the case table, the reference, the bounds).

Each case runs the C ABI directly, with every output buffer filled with a NaN bit pattern, padded leading dimensions where the ABI
takes them (the mha entry points) and one guard row after the last sample: every owned element must be written, every pad column
and guard row must keep its bits.  Values: O, lse, dQ, dK, dV (the packed [B*L, 3C] gradient included), dqkv, dbias_table and the
fused column sums against the same formulas in fp64 on the bf16 inputs,
  |got - ref| <= U |ref| + sum_c C_c * term_c
with the terms of attention64() named after the rounding each covers:
  C_S   the fp32 score (scale q k^T + bias + mask, folded into log2 units) and exp2 / lse, in units of P * E, E = A + |s|
  C_PV  P (times the dropout factor) rounded to bf16 for the PV / P^T dO MFMAs and their fp32 accumulation
  C_DS  dS rounded to bf16 for the dQ / dK MFMAs, and delta taken from the stored bf16 O
  C_SUM fp32 sums over windows (dbias_table) and rows (column sums)
The constants were set on the first MI355X run as the smallest power of two that passes every case; they are not to be raised to
admit a change.  FIBER_ATTN_CALIBRATE=<file> writes, per constant, the largest value any element needed (the others held)."""
import json
import math
import os
import sys

import pytest
import torch

from tests import attn_cases as ac
from tests.hip_util import BF, DEV, assert_elementwise
from tests.mp_util import run_bounded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = ac.U
CONST = ac.CONST
_CAL = os.environ.get("FIBER_ATTN_CALIBRATE")
_needed = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from fiber_amd import lib
    lib.load()
    return lib


def check(name, got, ref, base, terms, row_mask=None, record=True):
    """assert_elementwise with bound = base + sum_c CONST[c] * terms[c] (row_mask: rows to leave out, see the callers)."""
    got = got.detach().to(torch.float64)
    if row_mask is not None:
        got, ref, base = got[row_mask], ref[row_mask], base[row_mask]
        terms = {c: t[row_mask] for c, t in terms.items()}
    bound = base.to(torch.float64) + sum(CONST[c] * t.to(torch.float64) for c, t in terms.items())
    if _CAL and record:
        err = (got - ref).abs()
        for c, t in terms.items():
            rest = base + sum(CONST[o] * x for o, x in terms.items() if o != c)
            need = ((err - rest) / t.clamp_min(1e-300)).where(t > 0, torch.zeros_like(err)).max().item()
            _needed[c] = max(_needed.get(c, 0.0), need)
            _needed.setdefault("_worst", {})
            if need > _needed["_worst"].get(c, (0.0, ""))[0]:
                _needed["_worst"][c] = (need, name)
        with open(_CAL, "w") as f:
            json.dump(_needed, f, indent=1)
    return assert_elementwise(name, got, ref, bound)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def assert_written(name, buf, owned):
    """every element of buf[owned] (a bool mask of buf's shape) was written, every other element kept the fill pattern."""
    same = _bits(buf) == (ac.NAN_BF16 if buf.dtype == torch.bfloat16 else ac.NAN_F32)
    missed = int((same & owned).sum())
    stray = int((~same & ~owned).sum())
    assert missed == 0, f"{name}: {missed} owned elements never written (first at {torch.nonzero(same & owned)[0].tolist()})"
    assert stray == 0, f"{name}: {stray} elements written outside the owned region (first at {torch.nonzero(~same & ~owned)[0].tolist()})"


def _region(shape, rows, c0, c1, device=DEV):
    m = torch.zeros(shape, dtype=torch.bool, device=device)
    m[:rows, c0:c1] = True
    return m


def _canon_rows(x, B, L):          # [B, H, L, D] -> [B*L, H*D]
    return x.permute(0, 2, 1, 3).reshape(B * L, -1)


def _terms_rows(t, B, L):
    base, tt = t
    return _canon_rows(base, B, L), {c: _canon_rows(x, B, L) for c, x in tt.items()}


# ------------------------------------------------------------------------------------------------------------ window
def _window_checks(case, inp, o, dqkv, dtab, cs, ref, trm):
    B, H, W, heads = case["B"], case["H"], case["W"], case["heads"]
    rows, C = B * H * W, heads * 32
    cols = inp["cols"]
    n = case["name"]
    check(f"{n} O", o[:rows].view(rows, heads, 32), ref["o"], *trm["o"])
    for i, key in enumerate(("dq", "dk", "dv")):
        check(f"{n} {key}", dqkv[:rows][:, cols[i].reshape(-1)].view(rows, heads, 32), ref[key], *trm[key])
    check(f"{n} dbias_table", dtab, ref["dtable"], *trm["dtable"])
    if cs is not None:
        full = torch.zeros(rows, 3 * C, dtype=torch.float64, device=DEV)
        fb = {c: torch.zeros_like(full) for c in ("C_PV", "C_S", "C_DS")}
        fbase = torch.zeros_like(full)
        for i, key in enumerate(("dq", "dk", "dv")):
            full[:, cols[i].reshape(-1)] = ref[key].reshape(rows, -1)
            fbase[:, cols[i].reshape(-1)] = trm[key][0].reshape(rows, -1)
            for c, x in trm[key][1].items():
                fb[c][:, cols[i].reshape(-1)] = x.reshape(rows, -1)
        terms = {c: x.sum(0) for c, x in fb.items() if x.abs().sum() > 0}
        terms["C_SUM"] = full.abs().sum(0)
        check(f"{n} dqkv colsum", cs[:3 * C], full.sum(0), fbase.sum(0), terms)


@pytest.mark.parametrize("name", [c["name"] for c in ac.WIN_CASES])
def test_window_path(lib, name):
    """One window case: fp64 per-element bounds on O, dq / dk / dv, dbias_table and the fused column sums; the written region; two runs
    bit for bit equal; the backward with column sums writes the same dqkv as without."""
    case = ac.CASE_BY_NAME[name]
    inp = ac.make_window_inputs(case)
    B, H, W, heads, ws = case["B"], case["H"], case["W"], case["heads"], case["ws"]
    rows, C = B * H * W, heads * 32
    o, lse = ac.run_window_fwd(lib, case, inp)
    o2, lse2 = ac.run_window_fwd(lib, case, inp)
    assert torch.equal(_bits(o), _bits(o2)) and torch.equal(_bits(lse), _bits(lse2)), f"{name}: forward differs between two runs"
    assert_written(f"{name} o", o, _region(o.shape, rows, 0, C))
    lm = torch.zeros_like(lse, dtype=torch.bool)
    lm[:rows * heads] = True
    assert_written(f"{name} lse", lse, lm)
    dqkv, dtab, _ = ac.run_window_bwd(lib, case, inp, o, lse, colsum=False)
    dqkv2, dtab2, _ = ac.run_window_bwd(lib, case, inp, o, lse, colsum=False)
    assert torch.equal(_bits(dqkv), _bits(dqkv2)), f"{name}: dqkv differs between two runs"
    if ws * ws <= 336:
        assert torch.equal(_bits(dtab), _bits(dtab2)), f"{name}: dbias_table differs between two runs"
    # (the generic path, N > 336, folds dbias_table with atomicAdd in dbias_scatter_kernel: its summation order is free, so that output
    # is held to the bound only)
    assert_written(f"{name} dqkv", dqkv, _region(dqkv.shape, rows, 0, 3 * C))
    cs = None
    if case["colsum"]:
        dqkv3, dtab3, cs = ac.run_window_bwd(lib, case, inp, o, lse, colsum=True)
        assert torch.equal(_bits(dqkv3), _bits(dqkv)), f"{name}: dqkv with column sums differs"
        cm = torch.zeros_like(cs, dtype=torch.bool)
        cm[:3 * C] = True
        assert_written(f"{name} colsum", cs, cm)
    ref, trm = ac.window_reference(case, inp)
    _window_checks(case, inp, o, dqkv, dtab, cs, ref, trm)
    if case["inputs"] == "shift_dominant":
        # the masked keys still carry weight: a -inf shift mask (instead of Swin's additive -100) must fail
        bad, btrm = ac.window_reference(case, inp, mask_value=-math.inf)
        with pytest.raises(AssertionError):
            check(f"{name} O vs -inf mask", o[:rows].view(rows, heads, 32), bad["o"], *btrm["o"], record=False)


# ------------------------------------------------------------------------------------------------------------ mha / causal
def _all_min_rows(case):
    """[B*Lq] rows whose every key is masked with finfo(fp32).min: the reference's lse there is finfo.min itself (log L absorbed), a
    value no fp32 path stores; their O and gradients are checked, their lse only for being finite and shared by the backward."""
    B, Lq = case["B"], case["Lq"]
    m = torch.ones(B, Lq, dtype=torch.bool, device=DEV)
    if case["mask"] == "allmin":
        m[1] = False
    return m.reshape(-1)


@pytest.mark.parametrize("name", [c["name"] for c in ac.MHA_CASES + ac.CAUSAL_CASES])
def test_mha_path(lib, name):
    """One mha / causal case: fp64 per-element bounds on O, lse, dq, dk, dv; the written region of every output; two runs bit for bit
    equal; lse = NULL leaves O bit for bit unchanged."""
    case = ac.CASE_BY_NAME[name]
    inp = ac.make_mha_inputs(case)
    B, heads, Lq, Lk, D, ld = (case[k] for k in ("B", "heads", "Lq", "Lk", "D", "ld"))
    C = heads * D
    o, lse = ac.run_mha_fwd(lib, case, inp)
    o2, lse2 = ac.run_mha_fwd(lib, case, inp)
    o3, _ = ac.run_mha_fwd(lib, case, inp, lse=False)
    assert torch.equal(_bits(o), _bits(o2)) and torch.equal(_bits(lse), _bits(lse2)), f"{name}: forward differs between two runs"
    assert torch.equal(_bits(o), _bits(o3)), f"{name}: O with lse = NULL differs"
    assert_written(f"{name} o", o, _region(o.shape, B * Lq, 0, C))
    assert_written(f"{name} lse", lse, _region(lse.shape, B * Lq, 0, heads))
    g = ac.run_mha_bwd(lib, case, inp, o, lse)
    g2 = ac.run_mha_bwd(lib, case, inp, o, lse)
    for a, b in zip(g["buf"], g2["buf"]):
        assert torch.equal(_bits(a), _bits(b)), f"{name}: gradients differ between two runs"
    if case["packed"]:
        assert_written(f"{name} dqkv", g["buf"][0], _region(g["buf"][0].shape, B * Lq, 0, 3 * C))
    else:
        for key, buf, L in zip(("dq", "dk", "dv"), g["buf"], (Lq, Lk, Lk)):
            assert_written(f"{name} {key}", buf, _region(buf.shape, B * L, 0, C))
    keep = ac.dropout_keep(lib, case, inp) if case["p"] > 0 else None
    out, terms = ac.mha_reference(case, inp, keep)
    if keep is not None:                                     # (where P is 0 -- masked keys, causal -- the probe reads keep = 0)
        kept = keep[out["P"] > 1e-20].mean().item()
        assert 0.85 < kept < 0.95, kept
    check(f"{name} O", o[:B * Lq, :C], _canon_rows(out["O"], B, Lq), *_terms_rows(terms["O"], B, Lq))
    rows = _all_min_rows(case)
    lse_ref = out["lse"].permute(0, 2, 1).reshape(B * Lq, heads)
    lb, lt = terms["lse"]
    check(f"{name} lse", lse[:B * Lq], lse_ref, lb.permute(0, 2, 1).reshape(B * Lq, heads),
          {c: x.permute(0, 2, 1).reshape(B * Lq, heads) for c, x in lt.items()}, row_mask=rows)
    assert torch.isfinite(lse[:B * Lq]).all(), f"{name}: non-finite lse"
    for key, name_ref, L in (("dq", "dQ", Lq), ("dk", "dK", Lk), ("dv", "dV", Lk)):
        check(f"{name} {key}", g[key], _canon_rows(out[name_ref], B, L), *_terms_rows(terms[name_ref], B, L))


# ------------------------------------------------------------------------------------------------------------ refusals
def test_attention_refusals(lib):
    """FIBER_EINVAL for every shape / layout / argument contract the entry points state."""
    from fiber_amd.lib import FiberHipError
    z = lambda *s, dt=BF: torch.zeros(*s, dtype=dt, device=DEV)
    f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)

    def refused(fn, *args):
        with pytest.raises(FiberHipError, match="invalid argument"):
            lib.call(fn, *args)

    def wf(B, H, W, C, heads, ws, shift, lay):
        qkv, o, lse, tab = z(B * H * W, 3 * C), z(B * H * W, C), f(B * H * W * heads), f((2 * ws - 1) ** 2, heads)
        refused("fiber_window_attn_fwd_bf16", lib.ptr(qkv), lib.ptr(tab), lib.ptr(o), lib.ptr(lse), B, H, W, C, heads, ws, shift, lay)

    def wb(B, H, W, C, heads, ws, shift, lay, colsum=False):
        rows = B * H * W
        qkv, o, lse, tab = z(rows, 3 * C), z(rows, C), f(rows * heads), f((2 * ws - 1) ** 2, heads)
        cs, csw = (f(3 * C), f(64 * 3 * C)) if colsum else (None, None)
        part = f(max(1, lib.plain("fiber_window_attn_bwd_slices", max(1, rows // (ws * ws)), heads)) * heads * ws ** 4)
        refused("fiber_window_attn_bwd_bf16", lib.ptr(qkv), lib.ptr(tab), lib.ptr(o), lib.ptr(o), lib.ptr(lse), lib.ptr(z(rows, 3 * C)),
                lib.ptr(f((2 * ws - 1) ** 2, heads)), lib.ptr(f(rows * heads)), lib.ptr(part), lib.ptr(cs), lib.ptr(csw), B, H, W, C, heads,
                ws, shift, lay)

    wf(1, 14, 14, 64, 3, 7, 0, 0)            # C != heads * 32
    wb(1, 14, 14, 64, 3, 7, 0, 0)
    wf(1, 14, 15, 64, 2, 7, 0, 0)            # Wres % ws
    wb(1, 15, 14, 64, 2, 7, 0, 0)            # Hres % ws
    wf(1, 14, 14, 64, 2, 7, 7, 0)            # shift >= ws
    wb(1, 14, 14, 64, 2, 7, 7, 0)
    wf(1, 14, 14, 64, 2, 7, -1, 0)
    for lay in (-1, 5):                      # layouts outside 0..4
        wf(1, 14, 14, 64, 2, 7, 0, lay)
        wb(1, 14, 14, 64, 2, 7, 0, lay)
    wf(1, 14, 14, 64, 2, 7, 0, 3)            # the planar probe layouts: 12 x 12 windows only
    wb(1, 14, 14, 64, 2, 7, 0, 4)
    for lay in (1, 2):                       # the generic window path (N > 336) reads the reference layout only ...
        wf(1, 19, 19, 64, 2, 19, 0, lay)
        wb(1, 19, 19, 64, 2, 19, 0, lay)
    wb(1, 19, 19, 64, 2, 19, 0, 0, colsum=True)   # ... and has no fused column sums
    assert lib.plain("fiber_window_attn_colsum_rows", 1, 2, 19) == 0

    def mf(fn, B, heads, Lq, Lk, D, ldq, ldk, ldv, ldo, p=0.0):
        q, k, v, o, lse = z(B * Lq, ldq), z(B * Lk, ldk), z(B * Lk, ldv), z(B * Lq, ldo), f(B * Lq * heads)
        refused(fn, lib.ptr(q), lib.ptr(k), lib.ptr(v), None, lib.ptr(o), lib.ptr(lse), B, heads, Lq, Lk, D, ldq, ldk, ldv, ldo, D ** -0.5,
                p, 1, None)

    def mb(fn, B, heads, Lq, Lk, D, ld, lddq, lddk, lddv, p=0.0):
        q, k, o, lse = z(B * Lq, ld), z(B * Lk, ld), z(B * Lq, ld), f(B * Lq * heads)
        dq, dk, dv = z(B * Lq, max(lddq, 1)), z(B * Lk, max(lddk, 1)), z(B * Lk, max(lddv, 1))
        refused(fn, lib.ptr(q), lib.ptr(k), lib.ptr(k), None, lib.ptr(o), lib.ptr(o), lib.ptr(lse), lib.ptr(dq), lib.ptr(dk), lib.ptr(dv),
                lib.ptr(f(B * Lq * heads)), B, heads, Lq, Lk, D, ld, ld, ld, ld, ld, lddq, lddk, lddv, D ** -0.5, p, 1, None)

    for fn in ("fiber_mha_fwd_bf16", "fiber_mha_causal_fwd_bf16"):
        for D in (16, 48, 128):              # head_dim outside {32, 64}
            mf(fn, 2, 2, 16, 16, D, 2 * D, 2 * D, 2 * D, 2 * D)
        mf(fn, 2, 2, 16, 16, 32, 68, 64, 64, 64)     # ldq % 8
        mf(fn, 2, 2, 16, 16, 32, 64, 68, 64, 64)     # ldk % 8
        mf(fn, 2, 2, 16, 16, 32, 64, 64, 68, 64)     # ldv % 8
    mf("fiber_mha_fwd_bf16", 2, 2, 16, 16, 32, 64, 64, 64, 66)          # ldo % 4
    mf("fiber_mha_causal_fwd_bf16", 2, 2, 16, 16, 32, 64, 64, 64, 68)   # ldo % 8 (causal)
    for fn in ("fiber_mha_bwd_bf16", "fiber_mha_causal_bwd_bf16"):
        for D in (16, 128):
            mb(fn, 2, 2, 16, 16, D, 2 * D, 2 * D, 2 * D, 2 * D)
        mb(fn, 2, 2, 16, 16, 32, 68, 64, 64, 64)
        mb(fn, 2, 2, 16, 16, 32, 64, 66, 64, 64)     # lddq % 4
        mb(fn, 2, 2, 16, 16, 32, 64, 64, 66, 64)
        mb(fn, 2, 2, 16, 16, 32, 64, 64, 64, 66)
    mb("fiber_mha_causal_bwd_bf16", 2, 2, 16, 16, 32, 64, 68, 64, 64)   # causal: every leading dimension % 8
    # causal: Lq != Lk, L > 64, p_drop >= 1 (and < 0)
    mf("fiber_mha_causal_fwd_bf16", 2, 2, 16, 20, 64, 128, 128, 128, 128)
    mb("fiber_mha_causal_bwd_bf16", 2, 2, 16, 20, 64, 128, 128, 128, 128)
    mf("fiber_mha_causal_fwd_bf16", 2, 2, 65, 65, 32, 64, 64, 64, 64)
    mb("fiber_mha_causal_bwd_bf16", 2, 2, 65, 65, 32, 64, 64, 64, 64)
    for p in (1.0, 1.5, -0.1):
        mf("fiber_mha_causal_fwd_bf16", 2, 2, 40, 40, 64, 128, 128, 128, 128, p=p)
        mb("fiber_mha_causal_bwd_bf16", 2, 2, 40, 40, 64, 128, 128, 128, 128, p=p)
    mf("fiber_mha_fwd_bf16", 2, 2, 0, 16, 32, 64, 64, 64, 64)          # empty sides
    mf("fiber_mha_fwd_bf16", 2, 2, 16, 0, 32, 64, 64, 64, 64)


# ------------------------------------------------------------------------------------------------------------ probe
def test_attn_paths_probe_names_the_declared_kernels():
    """tools/probes/attn_paths.py runs every case (forward and backward) once under torch.profiler in a child: each launched exactly the
    kernels it declares, and every template the table names was reached."""
    r = run_bounded([sys.executable, os.path.join(ROOT, "tools", "probes", "attn_paths.py")], 300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    seen = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert set(seen) == set(ac.CASE_BY_NAME), sorted(set(ac.CASE_BY_NAME) ^ set(seen))
    wrong = {}
    for n, got in seen.items():
        c = ac.CASE_BY_NAME[n]
        want = {"fwd": sorted(set(c["fwd"])), "bwd": sorted(set(c["bwd"]))}
        if got != want:
            wrong[n] = (want, got)
    assert not wrong, json.dumps(wrong, indent=1)
