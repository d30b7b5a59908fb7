"""Every GEMM kernel path, element by element against fp64.

NT (gemm.hip): each (kernel template, epilogue) pair of tests/gemm_cases.py against the same formula in fp64 on the bf16 operands,
  |got - ref| <= [bf16 roundings the epilogue performs] + C_ACC * (|X| |W|^T) * |epilogue slope|
where the roundings are the ones the kernels are written to do: the output store (2^-8 |ref|), the branch before a residual is added
(2^-8 |branch|), the pre-activation before GELU (2^-8 |pre|, through gelu'), the accumulator before gelu' * aux (2^-8 |acc|), and the
documented GELU approximations (GELU_FWD_ERR, GELU_BWD_ERR).  C_ACC bounds the fp32 accumulation: set on the first MI355X run as the
smallest power of two that passes every case; it is not to be raised to admit a change.
TN (gemm_tn.hip): dW and the bias sums in fp32 against fp64, 2^-22 |ref| + C_TN * (|dY|^T |X|), at both tiles and every fold width.
GELU: the exact bf16 grid of [-12, 12] through the fused epilogues and the element-wise backward kernels."""
import json
import math
import os
import sys

import pytest
import torch

from tests import gemm_cases as gc
from tests.hip_util import BF, DEV, abs_mm64, assert_elementwise, mm64
from tests.mp_util import run_bounded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -8                 # bf16 store: |bf16(v) - v| <= 2^-8 |v|
C_ACC = 2.0 ** -24            # fp32 accumulation of the NT kernels, in units of |X| |W|^T (first MI355X run: 2^-24.33 needed, pre of stream-fc1)
C_TN = 2.0 ** -24             # the same for the TN kernel and its fold, in units of |dY|^T |X| (first MI355X run: 2^-24.51 needed)
C_SUM = 2.0 ** -16            # fp32 column sums of a stored bf16 output, in units of the column sums of |output|
GELU_FWD_ERR = 2.0 ** -20     # common.h gelu2_exact: |err| <= 8e-7 (A&S 7.1.28)
GELU_BWD_ERR = 2.0 ** -12     # common.h gelu_grad2: clamped minimax polynomial, |err| <= 1.7e-4 (1.9e-4 at the +-4.5 clamp)
ROWS = 32768                  # reference row block


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from fiber_amd import lib, ops
    lib.load()
    return ops


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.5 ** 0.5))


def dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x * 0.5 ** 0.5)) + x * torch.exp(-0.5 * x * x) * (2 * math.pi) ** -0.5


def _row_scale(case, inp, i, j):
    if "rowscale" not in inp:
        return 1.0
    m = torch.arange(i, j, device=DEV)
    return inp["rowscale"].double()[m // case["rps"]][:, None]


def nt_checks(case, inp, out, i, j):
    """(name, got, ref, base bound, accumulation term) for rows [i, j) of one NT case: bound = base + C_ACC * term."""
    f = gc.EPILOGUES[case["epi"]]
    x, w = inp["x"][i:j], inp["w"]
    A, AW = mm64(x, w), abs_mm64(x, w) * (1 + U)
    s = _row_scale(case, inp, i, j)
    b = inp["bias"].double() if "bias" in inp else 0.0
    y = out["y"][i:j]
    if "d" in f:                                             # s * bf16(acc) * gelu'(aux)
        gp = dgelu64(inp["aux"][i:j].double())
        ref = s * A * gp
        return [("y", y, ref, U * ref.abs() + s * (U * gp.abs() + GELU_BWD_ERR * (1 + U)) * A.abs(), s * gp.abs() * AW)]
    if "f" in f:                                             # fp32 output: acc + bias, no rounding but the accumulation
        ref = A + b
        return [("y fp32", y, ref, 2.0 ** -23 * ref.abs(), AW)]
    if "t" in f:                                             # fp32 stream: bf16(s (acc + b)) + R32 in fp32, its bf16 shadow
        br = s * (A + b)
        ref = br + inp["res32"][i:j].double()
        base32 = U * br.abs() + 2.0 ** -23 * ref.abs()
        return [("y32", out["y32"][i:j], ref, base32, s * AW), ("y shadow", y, ref, U * ref.abs() + base32, s * AW)]
    if "g" in f:                                             # s * gelu(bf16(acc + b)) (+ R)
        pre = A + b
        slope = dgelu64(pre).abs() + 0.8 * (U * pre.abs() + 2 * C_ACC * AW)       # |gelu''| <= 0.8 over the perturbation
        br = s * gelu64(pre)
        ref = br + inp["residual"][i:j].double() if "r" in f else br
        base = U * ref.abs() + s * (slope * U * pre.abs() + GELU_FWD_ERR) + (U * br.abs() if "r" in f else 0.0)
        res = [("y", y, ref, base, s * slope * AW)]
        if "p" in f:
            p = out["pre"][i:j]
            res.append(("pre", p, pre, U * pre.abs(), AW))
            if not case["kernel"].startswith("reg"):             # (the register-staged kernel takes GELU of the fp32 sum)
                brp = s * gelu64(p.double())                      # GELU of the stored bf16 pre-activation, as the epilogue does it
                refp = brp + inp["residual"][i:j].double() if "r" in f else brp
                res.append(("y = gelu(pre)", y, refp, U * refp.abs() + s * GELU_FWD_ERR + (U * brp.abs() if "r" in f else 0.0),
                            torch.zeros_like(refp)))
        return res
    br = s * (A + b)                                         # s (acc + b) (+ R: the branch rounded first)
    if "r" in f:
        ref = br + inp["residual"][i:j].double()
        return [("y", y, ref, U * ref.abs() + U * br.abs(), s * AW)]
    return [("y", y, br, U * br.abs(), s * AW)]


def check_nt_case(case, inp, out, c_acc=C_ACC):
    for i in range(0, case["M"], ROWS):
        j = min(case["M"], i + ROWS)
        for name, got, ref, base, term in nt_checks(case, inp, out, i, j):
            assert_elementwise(f"{case['name']} {name}", got, ref, base + c_acc * term, row0=i)
    if "colsum" in out:                                      # the bias gradient: column sums of the STORED output
        y = out["y"].double()
        assert_elementwise(f"{case['name']} colsum", out["colsum"], y.sum(0), C_SUM * y.abs().sum(0))


@pytest.mark.parametrize("name", [c["name"] for c in gc.CASES])
def test_gemm_nt_path(ops, name):
    """One (kernel, epilogue) pair: fp64 per-element bound, and two runs bit for bit equal."""
    case = gc.CASE_BY_NAME[name]
    inp = gc.make_inputs(case)
    out = gc.run(ops, case, inp)
    out2 = gc.run(ops, case, inp)
    for k in out:
        assert torch.equal(out[k], out2[k]), f"{name}: {k} differs between two runs"
    del out2
    check_nt_case(case, inp, out)


def test_gemm_row_tile_is_the_launched_tile(ops):
    """colpart is sized by fiber_gemm_row_tile: it must name the row tile of the kernel the column-sum call launches (the probe test
    below proves which kernel that is)."""
    from fiber_amd import lib
    tile = {"r256": 256, "r128": 128, "r64": 64}
    for c in gc.CASES:
        if "c" in gc.EPILOGUES[c["epi"]]:
            assert lib.plain("fiber_gemm_row_tile", c["M"], c["N"], c["K"]) == tile[c["kernel"]], c["name"]
    # the wide-shape rule alone used to answer 256 here: the 128x128 kernel then wrote ceil(M/128) rows into ceil(M/256)
    assert lib.plain("fiber_gemm_row_tile", 65536, 512, 128) == 128
    assert lib.plain("fiber_gemm_row_tile", 65536, 512, 192) == 128
    assert lib.plain("fiber_gemm_row_tile", 65536, 512, 256) == 256


def test_gemm_nt_rejects(ops):
    """The ABI's refusals: K % 8, N % 4, gelu' * aux with a residual, column sums with K % 64."""
    from fiber_amd.lib import FiberHipError
    x, w = torch.ones(256, 36, dtype=BF, device=DEV), torch.ones(64, 36, dtype=BF, device=DEV)
    with pytest.raises(FiberHipError):
        ops.gemm_nt(x, w)
    x, w = torch.ones(256, 64, dtype=BF, device=DEV), torch.ones(130, 64, dtype=BF, device=DEV)
    with pytest.raises(FiberHipError):
        ops.gemm_nt(x, w)
    w = torch.ones(64, 64, dtype=BF, device=DEV)
    h = torch.ones(256, 64, dtype=BF, device=DEV)
    with pytest.raises(FiberHipError):
        ops.gemm_nt(x, w, None, h, 2, aux=h)
    x, w = torch.ones(256, 72, dtype=BF, device=DEV), torch.ones(64, 72, dtype=BF, device=DEV)
    with pytest.raises(FiberHipError):
        ops.gemm_nt(x, w, None, None, 2, aux=h, want_colsum=True)


def test_gemm_paths_probe_names_the_declared_kernels():
    """tools/probes/gemm_paths.py runs every case once under torch.profiler in a child: each case launched the template it declares,
    and every kernel of the matrix was reached."""
    r = run_bounded([sys.executable, os.path.join(ROOT, "tools", "probes", "gemm_paths.py")], 300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    seen = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert set(seen) == set(gc.CASE_BY_NAME), sorted(set(gc.CASE_BY_NAME) ^ set(seen))
    wrong = {n: (gc.expected_kernel(gc.CASE_BY_NAME[n]), k) for n, k in seen.items()
             if not any(gc.expected_kernel(gc.CASE_BY_NAME[n]) in s for s in k)}
    assert not wrong, wrong
    families = {fam for fam in gc.FAMILIES.values() if any(fam in k for ks in seen.values() for k in ks)}
    assert families == set(gc.FAMILIES.values()), set(gc.FAMILIES.values()) - families


# ---- TN: dW = dY^T X (+ bias sums), csrc/gemm_tn.hip ---------------------------------------------------------------------------------
# (M, N, K, bias, DropPath rows per sample or None, row map): tile 128 (N or K < 192) and 256; one split and S > 1 for each fold width
# (tn_fold_ql: S < 16 -> 4, S < 64 -> 8, else 16); ragged M, N and K against the tiles; X row-strided
TN_CASES = [
    (448, 136, 104, False, None, False), (448, 136, 104, True, None, True), (3000, 136, 104, True, None, False),
    (3200, 136, 104, True, 640, False), (20000, 136, 104, False, None, True), (20480, 136, 104, True, 2048, False),
    (40000, 136, 104, True, None, False), (40960, 136, 104, False, 4096, True),
    (448, 264, 200, True, None, False), (448, 264, 200, False, 64, True), (3000, 264, 200, False, None, True),
    (3200, 264, 200, True, 640, False), (20000, 264, 200, True, None, False), (20480, 264, 200, False, 2048, True),
    (40000, 264, 200, True, None, True), (40960, 264, 200, True, 4096, False),
]


def _fold_ql(S):
    return 1 if S == 1 else 16 if S >= 64 else 8 if S >= 16 else 4


def _tn_inputs(M, N, K, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed + M + N + K)
    dy = (torch.randn(M, N, device=DEV, generator=g) + 0.25).to(BF)
    xs = torch.full((M, K + 24), float("nan"), device=DEV, dtype=BF)
    xs[:, :K] = (torch.randn(M, K, device=DEV, generator=g) * torch.linspace(0.5, 2.0, K, device=DEV)).to(BF)
    return dy, xs[:, :K]


@pytest.mark.parametrize("M,N,K,bias,rps,rowmap", TN_CASES)
def test_wgrad_tn_path(ops, M, N, K, bias, rps, rowmap):
    from fiber_amd import lib
    S = lib.plain("fiber_gemm_tn_splits", M, N, K)
    tile = 256 if (N >= 192 and K >= 192) else 128
    assert _fold_ql(S) == {448: 1, 3000: 4, 3200: 4, 20000: 8, 20480: 8, 40000: 16, 40960: 16}[M], (M, N, K, S)
    dy, x = _tn_inputs(M, N, K)
    keep = torch.ones(M, dtype=torch.float64, device=DEV)
    mask, scale = None, 1.0
    if rps:
        mask = torch.full((M // rps,), 1.25, device=DEV)
        mask[1] = 0.0
        scale = 1.25
        keep = (mask.double()[torch.arange(M, device=DEV) // rps] != 0).double() * scale
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(N)).to(torch.int32).to(DEV) if rowmap else None
    res = ops.wgrad(dy, x, want_bias=bias, row_mask=mask, scale=scale, row_map=perm)
    res2 = ops.wgrad(dy, x, want_bias=bias, row_mask=mask, scale=scale, row_map=perm)
    dw, db = res if bias else (res, None)
    assert torch.equal(dw, res2[0] if bias else res2)
    dyk = dy.double() * keep[:, None]
    ref, term = mm64(dyk.t(), x.double().t()), abs_mm64(dyk.t(), x.double().t())
    refb, termb = dyk.sum(0), dyk.abs().sum(0)
    if perm is not None:
        inv = torch.empty_like(perm.long())
        inv[perm.long()] = torch.arange(N, device=DEV)
        ref, term, refb, termb = ref[inv], term[inv], refb[inv], termb[inv]
    assert_elementwise(f"dW tile {tile} S {S}", dw, ref, 2.0 ** -22 * ref.abs() + C_TN * term)
    if bias:
        assert torch.equal(db, res2[1])
        assert_elementwise(f"db tile {tile} S {S}", db, refb, 2.0 ** -22 * refb.abs() + C_TN * termb)


# ---- GELU: the whole bf16 grid of [-12, 12] --------------------------------------------------------------------------------------------
def _bf16_grid():
    v = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float()
    v = v[torch.isfinite(v) & (v.abs() <= 12)]
    return torch.unique(v).to(BF).to(DEV)                   # every bf16 value in [-12, 12] (+-0 once)


def _ulp(v):
    a = v.abs()
    return torch.where(a > 0, torch.exp2(torch.floor(torch.log2(a.clamp_min(1e-300))) - 7), torch.zeros_like(a))


def _one_hot(M, K):
    x = torch.zeros(M, K, device=DEV, dtype=BF)
    x[torch.arange(M, device=DEV), torch.arange(M, device=DEV) % K] = 1
    return x


@pytest.mark.parametrize("M", [25600, 6144], ids=["q8", "ring128"])
def test_gelu_fwd_epilogue_sweep(ops, M):
    """fc1 epilogue with one-hot X rows and every bf16 value of [-12, 12] in W (bias 0): the pre-activation is exactly that value, and
    y = gelu(pre) within 1 bf16 ulp + 2^-20 of fp64 erf GELU (q8 at M = 25600, the 128x128 ring kernel at M = 6144)."""
    N, K = 512, 128
    grid = _bf16_grid()
    w = grid[torch.arange(N * K, device=DEV) % grid.numel()].view(N, K)
    x = _one_hot(M, K)
    y, pre = ops.gemm_nt(x, w, torch.zeros(N, device=DEV), None, 1, True)
    assert torch.equal(pre, w.t()[torch.arange(M, device=DEV) % K])
    ref = gelu64(pre.double())
    assert_elementwise(f"gelu fwd (M = {M})", y, ref, _ulp(ref) + GELU_FWD_ERR)


@pytest.mark.parametrize("M", [25600, 6144], ids=["q8", "ring128"])
@pytest.mark.parametrize("dy_one", [True, False])
def test_gelu_bwd_epilogue_sweep(ops, M, dy_one):
    """gelu' * aux epilogue with an accumulator of exactly dY (one-hot X, W constant along K) and aux sweeping the bf16 grid:
    within 1 bf16 ulp + 2^-12 |dY| of fp64 (q8 at M = 25600, the 128x128 ring kernel at M = 6144)."""
    N, K = 512, 128
    grid = _bf16_grid()
    aux = grid[torch.arange(M * N, device=DEV) % grid.numel()].view(M, N)
    dyv = torch.ones(N, device=DEV) if dy_one else ((torch.arange(N, device=DEV) % 13) * 0.25 - 1.375)
    w = dyv[:, None].expand(N, K).contiguous().to(BF)
    y, _ = ops.gemm_nt(_one_hot(M, K), w, None, None, 2, False, aux=aux)
    ref = dyv.double()[None, :] * dgelu64(aux.double())
    assert_elementwise(f"gelu' * aux (M = {M}, dY {'1' if dy_one else 'varied'})", y, ref, _ulp(ref) + GELU_BWD_ERR * dyv.double().abs()[None, :])


@pytest.mark.parametrize("dy_one", [True, False])
def test_gelu_bwd_elementwise_sweep(ops, dy_one):
    """fiber_gelu_bwd_bf16 and fiber_gelu_bwd_colsum_bf16 on the bf16 grid: dh within 1 ulp + 2^-12 |dY|, the column sums of the stored
    dh within C_SUM."""
    from fiber_amd import lib
    grid = _bf16_grid()
    M, N = 4104, 520                                        # 8 full / a partial column block and row slab
    h = grid[torch.arange(M * N, device=DEV) % grid.numel()].view(M, N)
    dg = torch.ones(M, N, device=DEV, dtype=BF) if dy_one else \
        (((torch.arange(M * N, device=DEV) % 11) * 0.375 - 1.75).view(M, N)).to(BF)
    ref = dg.double() * dgelu64(h.double())
    bound = _ulp(ref) + GELU_BWD_ERR * dg.double().abs()
    dh = torch.empty_like(h)
    lib.call("fiber_gelu_bwd_bf16", lib.ptr(dg), lib.ptr(h), lib.ptr(dh), M * N)
    assert_elementwise("fiber_gelu_bwd_bf16", dh, ref, bound)
    dh2, db = ops.gelu_bwd_colsum(dg, h)
    assert torch.equal(dh2, dh)
    assert_elementwise("fiber_gelu_bwd_colsum_bf16 colsum", db, dh.double().sum(0), C_SUM * dh.double().abs().sum(0))
