"""Exact cases for the K-loop structure of gemm_nt_q8_kernel: the seeded first K tile, the steady loop of the K tiles 1 .. nk - 3, the general
code of the last two, and the cursor's walk from one output tile of a workgroup into the next (stepped tile coordinates, per-lane offsets that
are recomputed only for a tile that is ragged in M or reaches past N).

As in tests/test_hip_gemm_mfma_shape.py the operands are small integers (or multiples of 1/8), every product and every partial sum is exact in
fp32 whatever the order, and the stored result is exact in its output format: the outputs must EQUAL the numpy reference, whose magnitudes are
asserted on the CPU.  Every case is launched twice (bit for bit equal) and must have run gemm_nt_q8_kernel and nothing else.  The activated
GELU outputs take the element-wise bounds of tests/test_hip_gemm_paths.py.

Shapes (256 x 256 tiles on 256 workgroups, 32 per XCD, an XCD's run of tiles dealt round-robin to its workgroups):
  [16897, 1024]  67 x 4 = 268 tiles, runs of 34 / 33: two output tiles on the first workgroups of an XCD and one on the rest; one row in the
                 last row tile, which is the second tile of a workgroup that began with a full one (clamped offsets after full-tile ones)
  [33024, 1024]  129 x 4 = 516 tiles, runs of 65 / 64: three and two output tiles per workgroup
  [16385, 832]   65 x 4 = 260 tiles, a partial last tile column (whole waves past N); a workgroup's tiles lie 32 ids apart, i.e. in ONE tile
                 column here: two clamped tiles in a row on some workgroups
  [23041, 576]   91 x 3 = 273 tiles: a workgroup's second tile lies two tile columns further (mod 3), so some workgroups go from a full tile
                 to one that reaches past N and others from such a tile back to a full one
K = 128, 192 (nk = 2, 3: never steady), 256 (one steady K tile), 320 (two), 576 (six)."""
import numpy as np
import pytest
import torch

from tests.hip_util import BF, DEV, assert_elementwise
from tests.test_hip_gemm_mfma_shape import _tri, _twice_on_q8
from tests.test_hip_gemm_paths import GELU_BWD_ERR, GELU_FWD_ERR, U, dgelu64, gelu64

pytestmark = pytest.mark.gpu

RPS = 1000                                                   # rows per sample of the row scale
K_SWEEP = {f"m16897_n1024_k{k}": (16897, 1024, k) for k in (128, 192, 256, 320, 576)}
WALKS = {"m33024_n1024_k256": (33024, 1024, 256), "m16385_n832_k256": (16385, 832, 256), "m16385_n832_k320": (16385, 832, 320),
         "m23041_n576_k256": (23041, 576, 256)}
EPI_SHAPE = (16897, 1024, 320)


def _t(a, dt=torch.float32):
    return torch.from_numpy(a).to(DEV).to(dt)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from fiber_amd import lib, ops
    lib.load()
    return ops


def _tiles_per_workgroup(M, N):
    """(most, fewest) output tiles of a workgroup that has any: the tile walk of gemm_nt_q8_kernel on 256 workgroups."""
    tiles = -(-M // 256) * -(-N // 256)
    assert tiles >= 200, "below the persistent threshold: not a q8 shape"
    counts = [tiles // 8 + (1 if x < tiles % 8 else 0) for x in range(8)]
    per = [-(-(c - w) // 32) for c in counts for w in range(32) if w < c]
    return max(per), min(per)


def int_case(M, N, K):
    """Integer NT operands and references (numpy, CPU): X, W in {-1, 0, 1}; bias[n] = n % 61 - 30, a distinct integer per column of a wave's
    64; scale in {0, 1, 2} per sample; integer residuals (bf16 and fp32)."""
    rng = np.random.default_rng(M + N + K)
    x = _tri(rng, (M, K), 0.5).astype(np.float32)
    w = _tri(rng, (N, K), 0.5).astype(np.float32)
    bias = (np.arange(N) % 61 - 30).astype(np.float32)
    scale = (np.arange(-(-M // RPS)) % 3).astype(np.float32)
    res = rng.integers(-40, 41, (M, N)).astype(np.float32)
    acc = x @ w.T
    assert K < 2 ** 24 and np.abs(acc).max() <= 96           # exact integers in fp32 and, below 256, in bf16
    ref_bias = acc + bias
    # with the row scale the BRANCH s (acc + b) is rounded to bf16 before R is added: both stay integers <= 256
    branch = scale[np.arange(M) // RPS][:, None] * ref_bias
    ref_res = branch + res
    assert np.abs(ref_bias).max() <= 126 and np.abs(branch).max() <= 256 and np.abs(ref_res).max() <= 256
    return dict(M=M, N=N, K=K, x=_t(x, BF), w=_t(w, BF), bias=_t(bias), scale=_t(scale), res=_t(res, BF), res32=_t(res),
                ref_plain=_t(acc), ref_bias=_t(ref_bias), ref_res=_t(ref_res))


@pytest.fixture(scope="module", params=list(K_SWEEP) + list(WALKS))
def nt_int(request):
    M, N, K = {**K_SWEEP, **WALKS}[request.param]
    most, fewest = _tiles_per_workgroup(M, N)
    assert (most, fewest) == ((3, 2) if M == 33024 else (2, 1)), (most, fewest)
    return int_case(M, N, K)


@pytest.fixture(scope="module")
def epi_int():
    return int_case(*EPI_SHAPE)


@pytest.fixture(scope="module")
def epi_eighths():
    """Operands on the 1/8 grid (|x| <= 1/2): products are multiples of 1/64 and the pre-activation, below 4 in magnitude, is exact in bf16."""
    M, N, K = EPI_SHAPE
    rng = np.random.default_rng(M + 3 * N + K)
    x = (rng.integers(-4, 5, (M, K)) * (rng.random((M, K)) < 0.25)).astype(np.float32) / 8
    w = (rng.integers(-4, 5, (N, K)) * (rng.random((N, K)) < 0.25)).astype(np.float32) / 8
    bias = ((np.arange(N) % 9) - 4).astype(np.float32) / 8
    scale = (np.arange(-(-M // RPS)) % 3).astype(np.float32)
    acc = x @ w.T
    pre = acc + bias
    for v in (acc, pre):                                     # multiples of 1/64 below 4: at most 8 significant bits
        assert np.abs(v).max() < 4 and np.array_equal(v * 64, np.round(v * 64))
    aux = (rng.integers(-24, 25, (M, N)).astype(np.float32)) / 8
    return dict(M=M, N=N, K=K, x=_t(x, BF), w=_t(w, BF), bias=_t(bias), aux=_t(aux, BF), acc=_t(acc), pre=_t(pre), scale=_t(scale),
                srow=_t(scale[np.arange(M) // RPS][:, None].copy()))


def _equal(name, got, ref):
    bad = (got.float() != ref).nonzero()
    assert bad.numel() == 0, f"{name}: {bad.shape[0]} wrong elements, first at {bad[0].tolist()} = tile {[v // 256 for v in bad[0].tolist()]}"


def test_q8_loop_bias(ops, nt_int):
    """Y = X W^T + bias at every K-loop length and tile walk: equal to the integer product, column by column."""
    d = nt_int
    y, _ = _twice_on_q8(lambda: ops.gemm_nt(d["x"], d["w"], d["bias"]))
    _equal("y", y, d["ref_bias"])


def test_q8_epi_plain(ops, epi_int):
    """No bias: the first MFMAs of a tile are seeded with zero."""
    d = epi_int
    y, _ = _twice_on_q8(lambda: ops.gemm_nt(d["x"], d["w"]))
    _equal("y", y, d["ref_plain"])


def test_q8_epi_residual_rowscale(ops, epi_int):
    """Y = s (X W^T + bias) + R with s in {0, 1, 2} per sample and an integer residual: exact."""
    d = epi_int
    y, _ = _twice_on_q8(lambda: ops.gemm_nt(d["x"], d["w"], d["bias"], d["res"], rowscale=d["scale"], rows_per_sample=RPS))
    _equal("y", y, d["ref_res"])


def test_q8_epi_stream_rowscale(ops, epi_int):
    """The fp32 residual stream with a row scale: s (X W^T + bias) + R32 in fp32 and its bf16 shadow, both exact integers."""
    d = epi_int
    y16, y32 = _twice_on_q8(lambda: ops.gemm_nt(d["x"], d["w"], d["bias"], res32=d["res32"], rowscale=d["scale"], rows_per_sample=RPS))
    _equal("y32", y32, d["ref_res"])
    _equal("y shadow", y16, d["ref_res"])


def test_q8_epi_gelu_pre(ops, epi_eighths):
    """GELU + pre-activation copy on the 1/8 grid: Ypre equals the exact product + bias; Y = gelu(Ypre) within the fused-GELU bound."""
    d = epi_eighths
    y, pre = _twice_on_q8(lambda: ops.gemm_nt(d["x"], d["w"], d["bias"], None, 1, True))
    _equal("pre", pre, d["pre"])
    ref = gelu64(d["pre"].double())
    assert_elementwise("y = gelu(pre)", y, ref, U * ref.abs() + GELU_FWD_ERR)


def test_q8_epi_gelu_rowscale(ops, epi_eighths):
    """The same with the DropPath row scale: Y = s gelu(pre)."""
    d = epi_eighths
    y, pre = _twice_on_q8(lambda: ops.gemm_nt(d["x"], d["w"], d["bias"], None, 1, True, rowscale=d["scale"], rows_per_sample=RPS))
    _equal("pre", pre, d["pre"])
    s = d["srow"].double()
    ref = s * gelu64(d["pre"].double())
    assert_elementwise("y = s gelu(pre)", y, ref, U * ref.abs() + s * GELU_FWD_ERR)


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "rowscale"])
def test_q8_epi_gelu_grad_aux(ops, epi_eighths, scaled):
    """s acc gelu'(aux) with an exact accumulator (no bias in this epilogue): only the output store and the gelu' polynomial may differ."""
    d = epi_eighths
    kw = dict(rowscale=d["scale"], rows_per_sample=RPS) if scaled else {}
    y, _ = _twice_on_q8(lambda: ops.gemm_nt(d["x"], d["w"], None, None, 2, False, aux=d["aux"], **kw))
    s = d["srow"].double() if scaled else 1.0
    a64 = d["acc"].double()
    ref = s * a64 * dgelu64(d["aux"].double())
    assert_elementwise("y = s acc gelu'(aux)", y, ref, U * ref.abs() + s * GELU_BWD_ERR * (1 + U) * a64.abs())
