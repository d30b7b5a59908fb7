"""Exact, order-independent cases for the lane <-> element mapping of the two large GEMM kernels (gemm_nt_q8_kernel, the 256-tile
gemm_tn_kernel): what a change of MFMA shape can get wrong and a tolerance could blur.

Operands are small integers (or multiples of 1/8), so every product and every partial sum is exact in fp32 whatever the summation
order, and the stored result is exact in its output format: the outputs must EQUAL the reference.  The references are computed once on
the CPU in numpy (float32 matrix products of integers below 2^24 are exact) and their magnitudes are asserted there, so the exactness
does not rest on luck.  The activated GELU outputs take the element-wise bounds of tests/test_hip_gemm_paths.py."""
import numpy as np
import pytest
import torch

from tests.hip_util import BF, DEV, assert_elementwise
from tests.test_hip_gemm_paths import GELU_BWD_ERR, GELU_FWD_ERR, U, dgelu64, gelu64

pytestmark = pytest.mark.gpu

K_NT = 128                                                   # two K tiles: the seeded first MFMAs and the steady state both run
# 101 row tiles x 2 = 202 tiles (just over the persistent threshold), one row in the last; a partial last tile column (whole waves past N)
NT_SHAPES = {"m25601_n512": (25601, 512), "m16385_n832": (16385, 832)}
RPS = 1000                                                   # rows per sample of the row scale


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from fiber_amd import lib, ops
    lib.load()
    return ops


def _tri(rng, shape, p):
    """Entries of {-1, 0, 1}, non-zero with probability p."""
    return (rng.integers(0, 2, shape) * 2 - 1) * (rng.random(shape) < p)


@pytest.fixture(scope="module", params=list(NT_SHAPES))
def nt_int(request):
    """Integer NT operands and references (numpy, CPU): X, W in {-1, 0, 1}; bias[n] = n % 61 - 30, a distinct integer per column of a
    wave's 64; scale in {0, 1, 2} per sample; an integer residual."""
    M, N = NT_SHAPES[request.param]
    rng = np.random.default_rng(M + N)
    x = _tri(rng, (M, K_NT), 0.75).astype(np.float32)
    w = _tri(rng, (N, K_NT), 0.75).astype(np.float32)
    bias = (np.arange(N) % 61 - 30).astype(np.float32)
    scale = (np.arange(-(-M // RPS)) % 3).astype(np.float32)
    res = rng.integers(-40, 41, (M, N)).astype(np.float32)
    acc = x @ w.T
    assert np.abs(acc).max() <= K_NT                         # integers of magnitude <= 128: exact in bf16
    ref_bias = acc + bias
    assert np.abs(ref_bias).max() <= K_NT + 30
    # plain + bias is stored as is; with the row scale the BRANCH s (acc + b) is rounded to bf16 before R is added: both stay integers <= 256
    branch = scale[np.arange(M) // RPS][:, None] * ref_bias
    ref_res = branch + res
    assert np.abs(branch).max() <= 256 and np.abs(ref_res).max() <= 256
    t = lambda a, dt=torch.float32: torch.from_numpy(a).to(DEV).to(dt)
    return dict(M=M, N=N, x=t(x, BF), w=t(w, BF), bias=t(bias), scale=t(scale), res=t(res, BF), ref_bias=t(ref_bias), ref_res=t(ref_res))


@pytest.fixture(scope="module", params=list(NT_SHAPES))
def nt_eighths(request):
    """Operands on the 1/8 grid (|x| <= 1/2): products are multiples of 1/64 and the pre-activation, below 4 in magnitude, is exact in bf16."""
    M, N = NT_SHAPES[request.param]
    rng = np.random.default_rng(M + 3 * N)
    x = (rng.integers(-4, 5, (M, K_NT)) * (rng.random((M, K_NT)) < 0.5)).astype(np.float32) / 8
    w = (rng.integers(-4, 5, (N, K_NT)) * (rng.random((N, K_NT)) < 0.5)).astype(np.float32) / 8
    bias = ((np.arange(N) % 9) - 4).astype(np.float32) / 8
    acc = x @ w.T
    pre = acc + bias
    for v in (acc, pre):                                     # multiples of 1/64 below 4: at most 8 significant bits
        assert np.abs(v).max() < 4 and np.array_equal(v * 64, np.round(v * 64))
    aux = (rng.integers(-24, 25, (M, N)).astype(np.float32)) / 8
    t = lambda a, dt=torch.float32: torch.from_numpy(a).to(DEV).to(dt)
    return dict(M=M, N=N, x=t(x, BF), w=t(w, BF), bias=t(bias), aux=t(aux, BF), acc=t(acc), pre=t(pre))


def _kernels(fn):
    """fn() under torch.profiler (device activity only, as tools/probes/gemm_paths.py): its result and the kernel names it launched."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = sorted({e.name.replace("(anonymous namespace)::", "") for e in prof.events()
                    if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name
                    and "fillBuffer" not in e.name and "copyBuffer" not in e.name})
    return out, names


def _twice_on_q8(fn):
    """Two launches of fn, bit for bit equal, the second one under the profiler: it must have run gemm_nt_q8_kernel and nothing else."""
    first = fn()
    second, names = _kernels(fn)
    assert names and all("gemm_nt_q8_kernel<" in n for n in names), names
    for a, b in zip(first, second):
        if a is not None:
            assert torch.equal(a, b), "two launches differ"
    return first


def test_nt_integer_bias(ops, nt_int):
    """Y = X W^T + bias with integer operands: equal to the integer product, column by column (a permuted bias seed cannot pass)."""
    d = nt_int
    y, _ = _twice_on_q8(lambda: ops.gemm_nt(d["x"], d["w"], d["bias"]))
    bad = (y.float() != d["ref_bias"]).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} wrong elements, first at {bad[0].tolist()}"


def test_nt_integer_residual_rowscale(ops, nt_int):
    """Y = s (X W^T + bias) + R with s in {0, 1, 2} per sample and an integer residual: exact."""
    d = nt_int
    y, _ = _twice_on_q8(lambda: ops.gemm_nt(d["x"], d["w"], d["bias"], d["res"], rowscale=d["scale"], rows_per_sample=RPS))
    bad = (y.float() != d["ref_res"]).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} wrong elements, first at {bad[0].tolist()}"


def test_nt_gelu_pre(ops, nt_eighths):
    """GELU + pre-activation copy on the 1/8 grid: Ypre equals the exact product + bias; Y = gelu(Ypre) within the fused-GELU bound."""
    d = nt_eighths
    y, pre = _twice_on_q8(lambda: ops.gemm_nt(d["x"], d["w"], d["bias"], None, 1, True))
    bad = (pre.float() != d["pre"]).nonzero()
    assert bad.numel() == 0, f"pre: {bad.shape[0]} wrong elements, first at {bad[0].tolist()}"
    ref = gelu64(d["pre"].double())
    assert_elementwise("y = gelu(pre)", y, ref, U * ref.abs() + GELU_FWD_ERR)


def test_nt_gelu_grad_aux(ops, nt_eighths):
    """acc * gelu'(aux) with an exact accumulator (no bias in this epilogue): only the output store and the gelu' polynomial may differ."""
    d = nt_eighths
    y, _ = _twice_on_q8(lambda: ops.gemm_nt(d["x"], d["w"], None, None, 2, False, aux=d["aux"]))
    a64 = d["acc"].double()
    ref = a64 * dgelu64(d["aux"].double())
    assert_elementwise("y = acc * gelu'(aux)", y, ref, U * ref.abs() + GELU_BWD_ERR * (1 + U) * a64.abs())


# ---- TN: dW = dY^T X and the bias sums, integer operands: fp32 results are exact integers for any M < 2^24 ----------------------------
# (M, N, K, rows per sample of the mask or None, scale): ragged N / K / M with S > 1 (slabs + fold, zero-row last K tile); the same with
# dropped samples and a scale; 7 K tiles, below the 8-tile split minimum (S = 1)
TN_CASES = {"ragged_split": (4100, 200, 264, None, 1.0), "masked_split": (4096, 200, 264, 128, 2.0), "one_split": (448, 256, 256, None, 1.0)}


@pytest.fixture(scope="module", params=list(TN_CASES))
def tn_int(request):
    M, N, K, rps, scale = TN_CASES[request.param]
    rng = np.random.default_rng(M + N + K)
    m = np.arange(M)[:, None]
    dy = (_tri(rng, (M, N), 1.0) * (m % 7 == np.arange(N)[None, :] % 7)).astype(np.float32)      # column n lives on rows = n mod 7
    x = (_tri(rng, (M, K), 0.8) * (m % 5 != np.arange(K)[None, :] % 5)).astype(np.float32)       # column k is empty on rows = k mod 5
    keep = np.ones(M, np.float32)
    mask = None
    if rps:
        mask = np.full(M // rps, 1.0, np.float32)
        mask[[1, 7, 8, 30]] = 0.0
        keep = (mask[np.arange(M) // rps] != 0).astype(np.float32)
    dyk = dy * keep[:, None]
    ref = scale * (dyk.T @ x)
    refb = scale * dyk.sum(0)
    assert M < 2 ** 24 and np.abs(ref).max() <= scale * M and np.abs(refb).max() <= scale * M
    assert np.abs(ref).max() > 0 and len(np.unique(ref, axis=0)) == N and len(np.unique(ref, axis=1).T) == K     # rows and columns distinguishable
    t = lambda a, dt=torch.float32: torch.from_numpy(a).to(DEV).to(dt)
    return dict(M=M, N=N, K=K, dy=t(dy, BF), x=t(x, BF), mask=None if mask is None else t(mask), scale=scale, ref=t(ref), refb=t(refb),
                S1=request.param == "one_split")


def test_tn_integer(ops, tn_int):
    """dW and dbias equal the integer reference on the 256-tile kernel; two launches bit for bit equal."""
    from fiber_amd import lib
    d = tn_int
    S = lib.plain("fiber_gemm_tn_splits", d["M"], d["N"], d["K"])
    assert (S == 1) == d["S1"], S
    run = lambda: ops.wgrad(d["dy"], d["x"], want_bias=True, row_mask=d["mask"], scale=d["scale"])
    (dw, db), (dw2, db2) = run(), run()
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "two launches differ"
    bad = (dw != d["ref"]).nonzero()
    assert bad.numel() == 0, f"dW: {bad.shape[0]} wrong elements, first at {bad[0].tolist()}"
    bad = (db != d["refb"]).nonzero()
    assert bad.numel() == 0, f"dbias: {bad.shape[0]} wrong elements, first at {bad[0].tolist()}"
