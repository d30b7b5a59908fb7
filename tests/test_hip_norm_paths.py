"""Every LayerNorm-family kernel path, element by element against fp64 (tests/norm_cases.py: the case table, the reference, the bounds).

Each case runs the C ABI directly with every output NaN-filled and GUARD rows (elements) after it: every owned element must be
written, no guard may change (the backward's workspace included).  LayerNorm / PatchMerging: y, y32, mean, rstd, dx, dgamma, dbeta;
fused LN-Mlp: y, g (forward), dx, dh, xhat (backward); the _LnMlp parameter gradients from the kernels' dh / xhat / g.  Two runs of
every case are bit-for-bit equal (dgamma / dbeta included: the fold has a fixed order).  The constants of norm_cases.CONST were set on
MI355X as the smallest power of two that passes every case; FIBER_NORM_CALIBRATE=<file> writes, per constant, the largest value
any element needed (the others held)."""
import json
import os
import sys

import pytest
import torch

from tests import norm_cases as nc
from tests.hip_util import BF, DEV, assert_elementwise, mm64, abs_mm64
from tests.mp_util import run_bounded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONST = nc.CONST
_CAL = os.environ.get("FIBER_NORM_CALIBRATE")
_needed = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from fiber_amd import lib
    lib.load()
    return lib


def check(name, got, ref, bound_spec, row0=0):
    """assert_elementwise with bound = base + sum_c CONST[c] * terms[c]."""
    base, terms = bound_spec
    got = got.detach().to(torch.float64)
    bound = base.to(torch.float64) + sum(CONST[c] * t.to(torch.float64) for c, t in terms.items())
    if _CAL:
        err = (got - ref).abs()
        for c, t in terms.items():
            rest = base + sum(CONST[o] * x for o, x in terms.items() if o != c)
            need = ((err - rest) / t.clamp_min(1e-300)).where(t > 0, torch.zeros_like(err)).max().item()
            if need > _needed.get(c, (0.0, ""))[0]:
                _needed[c] = (need, name)
        with open(_CAL, "w") as f:
            json.dump(_needed, f, indent=1)
    return assert_elementwise(name, got, ref, bound, row0=row0)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _nan(t):
    return _bits(t) == (nc.NAN_BF16 if t.dtype == torch.bfloat16 else nc.NAN_F32)


def assert_written(name, buf, n):
    """the first n rows (elements) of buf written, the rest (the guard) untouched"""
    missed = int(_nan(buf[:n]).sum())
    stray = int((~_nan(buf[n:])).sum())
    assert missed == 0, f"{name}: {missed} owned elements never written (first at {torch.nonzero(_nan(buf[:n]))[0].tolist()})"
    assert stray == 0, f"{name}: {stray} guard elements written"


def assert_same(name, a, b):
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{name}: {k} differs between two runs"


# ---- LayerNorm and PatchMerging --------------------------------------------------------------------------------------------------------
LN_CASES = [c["name"] for c in nc.CASES if c["kind"] != "mlp"]


@pytest.mark.parametrize("name", LN_CASES)
def test_layernorm_path(lib, name):
    case = nc.CASE_BY_NAME[name]
    inp = nc.make_ln_inputs(case)
    rows, C = case["rows"], nc.ln_width(case)
    f1 = nc.run_ln_fwd(lib, case, inp)
    b1 = nc.run_ln_bwd(lib, case, inp, f1)
    f2 = nc.run_ln_fwd(lib, case, inp)
    b2 = nc.run_ln_bwd(lib, case, inp, f2)
    assert_same(f"{name} fwd", f1, f2)
    assert_same(f"{name} bwd", {k: v for k, v in b1.items() if k != "ws"}, b2)
    del f2, b2
    for k in f1:
        assert_written(f"{name} {k}", f1[k], rows)
    assert_written(f"{name} dx", b1["dx"], inp["x"].shape[0])
    assert_written(f"{name} dgamma", b1["dgamma"], C)
    assert_written(f"{name} dbeta", b1["dbeta"], C)
    ws_n = b1["ws"].numel() - 64
    assert not bool((~_nan(b1["ws"][ws_n:])).any()), f"{name}: written past the workspace"

    xr = nc.ln_rows(case, inp)
    dx_rows = torch.empty(rows, C, dtype=torch.float64, device=DEV)
    dgamma = torch.zeros(C, dtype=torch.float64, device=DEV)
    dbeta = torch.zeros_like(dgamma)
    red = {"dgamma": [torch.zeros_like(dgamma), {}], "dbeta": [torch.zeros_like(dgamma), {}]}
    for i in range(0, rows, nc.ROWS):
        j = min(rows, i + nc.ROWS)
        out, bd = nc.ln_fwd_reference(xr[i:j], inp["gamma"], inp["beta"], case["eps"])
        check(f"{name} y", f1["y"][i:j], out["y"], bd["y"], i)
        if "y32" in f1:
            check(f"{name} y32", f1["y32"][i:j], out["y"], bd["y32"], i)
        check(f"{name} mean", f1["mean"][i:j, None], out["mean"][:, None], (bd["mean"][0][:, None], {"STAT": bd["mean"][1]["STAT"][:, None]}), i)
        check(f"{name} rstd", f1["rstd"][i:j, None], out["rstd"][:, None], (bd["rstd"][0][:, None], {"STAT": bd["rstd"][1]["STAT"][:, None]}), i)
        dres = inp["dres"][i:j] if "dres" in inp else None
        ob, bb = nc.ln_bwd_reference(xr[i:j], inp["dy"][i:j], inp["gamma"], f1["mean"][i:j], f1["rstd"][i:j], dres, case)
        dx_rows[i:j] = ob["dx"]
        if case["kind"] == "ln":
            check(f"{name} dx", b1["dx"][i:j], ob["dx"], bb["dx"], i)
        else:
            dx_bound = bb["dx"]
        dgamma += ob["dgamma"]
        dbeta += ob["dbeta"]
        for k in ("dgamma", "dbeta"):
            red[k][0] += bb[k][0]
            for c, t in bb[k][1].items():
                red[k][1][c] = red[k][1].get(c, 0) + t
    if case["kind"] == "ln":
        const = [r for r in nc.const_rows(rows)]
        if const:                                            # var = 0: xhat = 0, y = beta to the bit
            assert torch.equal(f1["y"][const], inp["beta"].to(BF)[None].expand(len(const), C)), f"{name}: constant rows"
    else:                                                    # PatchMerging: dx scattered back to the source tokens
        B, H, W, Cs = case["B"], case["H"], case["W"], case["C"]
        ref = nc.merge_scatter(dx_rows, B, H, W, Cs)
        base = nc.merge_scatter(dx_bound[0], B, H, W, Cs)
        terms = {c: nc.merge_scatter(t, B, H, W, Cs) for c, t in dx_bound[1].items()}
        check(f"{name} dx", b1["dx"][:B * H * W], ref, (base, terms))
    check(f"{name} dgamma", b1["dgamma"][:C, None], dgamma[:, None], (red["dgamma"][0][:, None], {c: t[:, None] for c, t in red["dgamma"][1].items()}))
    check(f"{name} dbeta", b1["dbeta"][:C, None], dbeta[:, None], (red["dbeta"][0][:, None], {c: t[:, None] for c, t in red["dbeta"][1].items()}))


# ---- fused LN-Mlp -------------------------------------------------------------------------------------------------------------------
MLP_CASES = [c["name"] for c in nc.CASES if c["kind"] == "mlp"]


@pytest.mark.parametrize("name", MLP_CASES)
def test_ln_mlp_path(lib, name):
    case = nc.CASE_BY_NAME[name]
    inp = nc.make_mlp_inputs(case)
    M, C = case["M"], case["C"]
    f1 = nc.run_mlp_fwd(lib, case, inp)
    f2 = nc.run_mlp_fwd(lib, case, inp, with_g=not case["g"])   # y does not depend on whether G is stored
    assert torch.equal(_bits(f1["y"]), _bits(f2["y"])), f"{name}: y with and without g differ"
    f2 = nc.run_mlp_fwd(lib, case, inp)
    assert_same(f"{name} fwd", f1, f2)
    b1 = nc.run_mlp_bwd(lib, case, inp)
    b2 = nc.run_mlp_bwd(lib, case, inp)
    assert_same(f"{name} bwd", b1, b2)
    del f2, b2
    for k, buf in list(f1.items()) + list(b1.items()):
        assert_written(f"{name} {k}", buf, M)
    for i in range(0, M, nc.ROWS):
        j = min(M, i + nc.ROWS)
        out, bd = nc.mlp_reference(case, inp, i, j)
        check(f"{name} y", f1["y"][i:j], out["y"], bd["y"], i)
        if "g" in f1:
            check(f"{name} g", f1["g"][i:j], out["g"], bd["g"], i)
        check(f"{name} xhat", b1["xhat"][i:j], out["xhat"], bd["xhat"], i)
        check(f"{name} dh", b1["dh"][i:j], out["dh"], bd["dh"], i)
        check(f"{name} dx", b1["dx"][i:j], out["dx"], bd["dx"], i)


def test_ln_mlp_parameter_gradients(lib):
    """ops._LnMlp's gradients of gamma, beta, W1, b1, W2, b2: the host-side unfold dW1 = dW1' diag(gamma) + db1 (x) beta,
    dgamma = colsum(dW1' * W1), dbeta = W1^T db1 on the kernels' own dh / xhat / g (each pinned above), against fp64."""
    from fiber_amd import ops
    B, L, C = 3, 192, 128                                   # (whole 64-row tiles a sample: dW2 takes the exact DropPath fold)
    H = 4 * C
    g = torch.Generator(device=DEV).manual_seed(11)
    x = ((torch.randn(B, L, C, device=DEV, generator=g) * 1.3 + 0.2)).to(BF).requires_grad_(True)
    gamma = (1 + 0.3 * torch.randn(C, device=DEV, generator=g))
    gamma[::7] = 0.0
    gamma[3::11] = -0.7
    beta = 0.2 * torch.randn(C, device=DEV, generator=g)
    w1 = (torch.randn(H, C, device=DEV, generator=g) * C ** -0.5).to(BF).float()
    b1 = 0.1 * torch.randn(H, device=DEV, generator=g) + torch.linspace(-0.5, 0.5, H, device=DEV)
    w2 = (torch.randn(C, H, device=DEV, generator=g) * H ** -0.5).to(BF).float()
    b2 = 0.1 * torch.randn(C, device=DEV, generator=g)
    params = [t.clone().requires_grad_(True) for t in (gamma, beta, w1, b1, w2, b2)]
    rs = torch.tensor([1.25, 0.0, 1.25], device=DEV)
    y = ops._LnMlp.apply(x, params[0], params[1], 1e-5, *params[2:], rs, 1.25)
    dy = torch.randn(B, L, C, device=DEV, generator=g).to(BF)
    y.backward(dy)
    # the kernels' operands of the weight-gradient GEMMs, as the backward produced them
    w1p, b1p, w2p, w2tp, w1tp = ops._ln_mlp_weights(params[0], params[1], params[2], params[3], params[4])
    M = B * L
    case = nc._mlp("unfold", C, M, rps=L)
    inp = dict(x=x.detach().view(M, C), dy=dy.view(M, C), w1p=w1p, b1p=b1p, w2p=w2p, w2tp=w2tp, w1tp=w1tp, b2=b2, rowscale=rs)
    f = nc.run_mlp_fwd(lib, case, inp, with_g=True)
    b = nc.run_mlp_bwd(lib, case, inp)
    dh, xh, G = b["dh"][:M].double(), b["xhat"][:M].double(), f["g"][:M].double()
    dW1p, adW1p = mm64(dh.t(), xh.t()), abs_mm64(dh.t(), xh.t())
    db1, adb1 = dh.sum(0), dh.abs().sum(0)
    w1d, gd, bd = w1.double(), gamma.double(), beta.double()
    s = rs.double().repeat_interleave(L)[:, None]
    dys = dy.view(M, C).double() * s
    CT = 2.0 ** -22                                           # fp32 TN GEMM + fold and the fp32 unfold: relative to the |.| sums
    want = {
        "dgamma": ((dW1p * w1d).sum(0), (adW1p * w1d.abs()).sum(0)),
        "dbeta": (w1d.t() @ db1, w1d.abs().t() @ adb1),
        "dW1": (dW1p * gd[None] + torch.outer(db1, bd), adW1p * gd.abs()[None] + torch.outer(adb1, bd.abs())),
        "db1": (db1, adb1),
        "dW2": (mm64(dys.t(), G.t()), abs_mm64(dys.t(), G.t())),
        "db2": (dys.sum(0), dys.abs().sum(0)),
    }
    for (k, (ref, term)), p in zip(want.items(), params):
        ref2 = ref if ref.dim() == 2 else ref[:, None]
        term2 = term if term.dim() == 2 else term[:, None]
        got = p.grad if p.grad.dim() == 2 else p.grad[:, None]
        assert_elementwise(f"_LnMlp {k}", got, ref2, CT * term2 + 2.0 ** -23 * ref2.abs())


# ---- ABI answers -------------------------------------------------------------------------------------------------------------------------
def _rc(lib, name, *args):
    return getattr(lib.load(), name)(*args, torch.cuda.current_stream().cuda_stream)


def test_norm_abi_refusals(lib):
    """C & 7, C > 4096, merged 4C > 3072, odd H or W, fused C outside {128, 256}, rowscale with M % rps != 0, fused M <= 0:
    FIBER_EINVAL; nothing launched."""
    P = lib.ptr
    x = torch.zeros(64 * 4104, dtype=BF, device=DEV)
    f = torch.zeros(16384, device=DEV)
    p = (P(x), P(f), P(f), P(x), P(f), P(f))
    assert _rc(lib, "fiber_layernorm_fwd_bf16", *p, 4, 100, 1e-5) == 1
    assert _rc(lib, "fiber_layernorm_fwd_bf16", *p, 4, 4104, 1e-5) == 1
    assert _rc(lib, "fiber_layernorm_fwd_stream", P(x), P(f), P(f), P(x), None, P(f), P(f), 4, 4104, 1e-5, 1) == 1
    assert _rc(lib, "fiber_layernorm_bwd_bf16", P(x), P(x), P(f), P(f), P(f), None, P(x), P(f), P(f), P(f), 4, 100) == 1
    assert _rc(lib, "fiber_layernorm_bwd_stream", P(x), P(x), P(f), P(f), P(f), None, P(x), P(f), P(f), P(f), 4, 4104, 1) == 1
    for C, H, W in ((776, 4, 4), (1024, 4, 4), (100, 4, 4), (128, 5, 4), (128, 4, 7)):
        assert _rc(lib, "fiber_patch_merge_ln_fwd_bf16", *p, 1, H, W, C, 1e-5) == 1, (C, H, W)
        assert _rc(lib, "fiber_patch_merge_ln_fwd_stream", *p, 1, H, W, C, 1e-5, 1) == 1, (C, H, W)
        assert _rc(lib, "fiber_patch_merge_ln_bwd_bf16", P(x), P(x), P(f), P(f), P(f), P(x), P(f), P(f), P(f), 1, H, W, C) == 1, (C, H, W)
        assert _rc(lib, "fiber_patch_merge_ln_bwd_stream", P(x), P(x), P(f), P(f), P(f), P(x), P(f), P(f), P(f), 1, H, W, C, 1) == 1
    for C, M, rs, rps in ((192, 64, None, 0), (64, 64, None, 0), (128, 100, P(f), 32), (128, 64, P(f), 0), (128, 0, None, 0),
                          (256, -32, None, 0)):
        assert _rc(lib, "fiber_ln_mlp_fwd_bf16", P(x), P(x), P(f), P(x), P(f), rs, P(x), None, M, C, rps, 1e-5) == 1, (C, M, rps)
        assert _rc(lib, "fiber_ln_mlp_bwd_bf16", P(x), P(x), P(x), P(f), P(x), P(x), rs, P(x), P(x), P(x), M, C, rps, 1e-5) == 1
    torch.cuda.synchronize()


def test_norm_zero_rows(lib):
    """rows = 0 (B = 0 for PatchMerging) at each of the eight LayerNorm entry points: FIBER_OK, nothing written."""
    P = lib.ptr
    bufs = [nc.nan_buf(4096, t, DEV) for t in (BF, torch.float32, torch.float32, BF, torch.float32, torch.float32, torch.float32)]
    y, mean, rstd, dx, dg, db, ws = bufs
    x, g = torch.ones(4096, dtype=BF, device=DEV), torch.ones(1024, device=DEV)
    assert _rc(lib, "fiber_layernorm_fwd_bf16", P(x), P(g), P(g), P(y), P(mean), P(rstd), 0, 128, 1e-5) == 0
    assert _rc(lib, "fiber_layernorm_fwd_stream", P(x), P(g), P(g), P(y), P(mean), P(mean), P(rstd), 0, 128, 1e-5, 1) == 0
    assert _rc(lib, "fiber_layernorm_bwd_bf16", P(x), P(x), P(g), P(g), P(g), P(x), P(dx), P(dg), P(db), P(ws), 0, 128) == 0
    assert _rc(lib, "fiber_layernorm_bwd_stream", P(x), P(x), P(g), P(g), P(g), None, P(dx), P(dg), P(db), P(ws), 0, 128, 1) == 0
    assert _rc(lib, "fiber_patch_merge_ln_fwd_bf16", P(x), P(g), P(g), P(y), P(mean), P(rstd), 0, 8, 8, 32, 1e-5) == 0
    assert _rc(lib, "fiber_patch_merge_ln_fwd_stream", P(x), P(g), P(g), P(y), P(mean), P(rstd), 0, 8, 8, 32, 1e-5, 1) == 0
    assert _rc(lib, "fiber_patch_merge_ln_bwd_bf16", P(x), P(x), P(g), P(g), P(g), P(dx), P(dg), P(db), P(ws), 0, 8, 8, 32) == 0
    assert _rc(lib, "fiber_patch_merge_ln_bwd_stream", P(x), P(x), P(g), P(g), P(g), P(dx), P(dg), P(db), P(ws), 0, 8, 8, 32, 1) == 0
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        assert bool(_nan(b).all()), f"buffer {i} written by a zero-row call"


# ---- launched kernels ------------------------------------------------------------------------------------------------------------------
def test_norm_paths_probe_names_the_declared_kernels():
    """tools/probes/norm_paths.py runs every case's forward and backward once under torch.profiler in a child: each launched the
    templates it declares, and nothing else."""
    r = run_bounded([sys.executable, os.path.join(ROOT, "tools", "probes", "norm_paths.py")], 300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    seen = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert set(seen) == set(nc.CASE_BY_NAME), sorted(set(nc.CASE_BY_NAME) ^ set(seen))
    wrong = {n: (nc.expected_kernels(nc.CASE_BY_NAME[n]), k) for n, k in seen.items()
             if {d: sorted(v) for d, v in nc.expected_kernels(nc.CASE_BY_NAME[n]).items()} != k}
    assert not wrong, wrong
