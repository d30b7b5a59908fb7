"""The 256-tile weight-gradient kernel walks its 64-row plan units as two 32-row K tiles over a ring of LDS stages, two wave groups one
phase apart (csrc/gemm_tn.hip).  What that loop can get wrong: a stage read before it landed or refilled before it was read (prologue
shorter than the ring, the last tiles of a split, dropped tiles that skip the math but not the ring), the halves of the last unit past M,
the sample counters in 32-row steps, and the 64-sample reload of the DropPath ballot.

Operands are integers of {-1, 0, 1} or multiples of 1/8 below 1/2 (tests/test_hip_gemm_mfma_shape.py): every product and partial sum is
exact in fp32 in any order, the numpy reference is exact, and dW / dbias must EQUAL it.  Every case is launched in four forms (bias sums
on / off, row_map on / off), each twice, bit for bit equal."""
import numpy as np
import pytest
import torch

from tests.hip_util import BF, DEV

pytestmark = pytest.mark.gpu

NK = {"256": (256, 256), "200x264": (200, 264)}              # one full tile; ragged N and K (two tile columns), both on the 256 tile

# name -> (M, rows per sample of the mask or None, dropped samples, scale, operand grid, splits the plan makes of it at both (N, K))
CASES = {}
for M in (32, 64, 96, 160):                                  # 1-3 plan units = 2-6 K tiles against 4 stages requested ahead, one split
    CASES[f"short_m{M}"] = (M, None, (), 1.0, "int", 1)
for r in (1, 31, 32, 33, 63):                                # the last unit: a partial first half and an empty second, a full first half, a partial second
    CASES[f"ragged_m{64 * 9 + r}"] = (64 * 9 + r, None, (), 1.0, "eighths" if r == 33 else "int", 1)
CASES["split_m4100"] = (4100, None, (), 1.0, "int", 8)       # 65 units in splits of 9: the last split has 2 units, 4 rows in its last
CASES["split_tail_m4632"] = (4632, None, (), 2.0, "eighths", 9)   # 73 units in splits of 9: the last split is ONE unit of 24 rows (2 tiles < ring)
# 64 samples of 64 rows (2 K tiles each) in 8 splits of 8; 8 samples of 576 rows (18 K tiles) in 9 splits of 8 units (samples straddle splits)
CASES["mask64_first"] = (4096, 64, (0,), 1.0, "int", 8)
CASES["mask64_last"] = (4096, 64, (63,), 1.0, "int", 8)
CASES["mask64_run"] = (4096, 64, tuple(range(10, 18)), 2.0, "int", 8)        # 16 dropped K tiles across a split boundary
CASES["mask64_kept"] = (4096, 64, (), 4.0, "eighths", 8)
CASES["mask576_first"] = (4608, 576, (0,), 1.0, "int", 9)
CASES["mask576_last"] = (4608, 576, (7,), 2.0, "int", 9)
CASES["mask576_run"] = (4608, 576, (2, 3), 1.0, "eighths", 9)
CASES["mask576_kept"] = (4608, 576, (), 0.5, "int", 9)

# 66 samples of 64 rows in ONE split (11 x 12 = 132 output tiles leave no room to split): the ballot of 64 samples is reloaded inside the loop
RELOAD = dict(M=66 * 64, N=2568, K=2824, rps=64, drop=(0, 5, 62, 63, 65), scale=2.0)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from fiber_amd import lib, ops
    lib.load()
    return ops


def _operands(M, N, K, rps, drop, scale, grid):
    """dY, X, mask on the device and the exact references (numpy, CPU) of dW and dbias."""
    rng = np.random.default_rng(M + 3 * N + 7 * K + len(drop))
    m = np.arange(M)[:, None]
    if grid == "int":
        dy = ((rng.integers(0, 2, (M, N)) * 2 - 1) * (m % 7 == np.arange(N)[None, :] % 7)).astype(np.float32)     # column n lives on rows = n mod 7
        x = ((rng.integers(0, 2, (M, K)) * 2 - 1) * (rng.random((M, K)) < 0.8) * (m % 5 != np.arange(K)[None, :] % 5)).astype(np.float32)
    else:
        dy = (rng.integers(-4, 5, (M, N)) * (rng.random((M, N)) < 0.5)).astype(np.float32) / 8
        x = (rng.integers(-4, 5, (M, K)) * (rng.random((M, K)) < 0.5)).astype(np.float32) / 8
    mask, keep = None, np.ones(M, np.float32)
    if rps:
        assert M % rps == 0
        mask = np.full(M // rps, 1.0, np.float32)
        mask[list(drop)] = 0.0
        keep = (mask[np.arange(M) // rps] != 0).astype(np.float32)
    dyk = dy * keep[:, None]
    acc, accb = dyk.T @ x, dyk.sum(0)
    # multiples of 1/64 below 2^22 / 64: exact in fp32 whatever the order, and still exact times the scales used (powers of two <= 4, so
    # that a split's scaled slab is exact as well)
    assert scale in (0.5, 1.0, 2.0, 4.0)
    assert np.abs(acc).max() * 64 < 2 ** 22 and np.array_equal(acc * 64, np.round(acc * 64)) and np.abs(acc).max() > 0
    ref, refb = np.float32(scale) * acc, np.float32(scale) * accb
    t = lambda a, dt=torch.float32: torch.from_numpy(a).to(DEV).to(dt)
    return dict(dy=t(dy, BF), x=t(x, BF), mask=None if mask is None else t(mask), scale=scale, ref=t(ref), refb=t(refb))


def _same(name, got, ref):
    bad = (got != ref).nonzero()
    assert bad.numel() == 0, f"{name}: {bad.shape[0]} wrong elements, first at {bad[0].tolist()}"


def _check(ops, d, N):
    perm = torch.from_numpy(np.random.default_rng(N).permutation(N).astype(np.int32)).to(DEV)
    inv = torch.empty(N, dtype=torch.long, device=DEV)
    inv[perm.long()] = torch.arange(N, device=DEV)           # row r of a permuted result is row inv[r] of the plain one
    for want_bias in (True, False):
        for row_map in (None, perm):
            run = lambda: ops.wgrad(d["dy"], d["x"], want_bias=want_bias, row_mask=d["mask"], scale=d["scale"], row_map=row_map)
            a, b = run(), run()
            (dw, db), (dw2, db2) = (a, b) if want_bias else ((a, None), (b, None))
            tag = f"bias={want_bias} row_map={row_map is not None}"
            assert torch.equal(dw, dw2) and (db is None or torch.equal(db, db2)), f"{tag}: two launches differ"
            _same(f"dW {tag}", dw, d["ref"] if row_map is None else d["ref"][inv])
            if want_bias:
                _same(f"dbias {tag}", db, d["refb"] if row_map is None else d["refb"][inv])


@pytest.mark.parametrize("nk", list(NK))
@pytest.mark.parametrize("case", list(CASES))
def test_tn_ring_exact(ops, case, nk):
    from fiber_amd import lib
    M, rps, drop, scale, grid, splits = CASES[case]
    N, K = NK[nk]
    assert lib.plain("fiber_gemm_tn_splits", M, N, K) == splits
    _check(ops, _operands(M, N, K, rps, drop, scale, grid), N)


def test_tn_ring_mask_reload(ops):
    """More than 64 samples in one split: samples 62 - 65 straddle the reload of the ballot (dropped, dropped, kept, dropped)."""
    from fiber_amd import lib
    c = RELOAD
    assert lib.plain("fiber_gemm_tn_splits", c["M"], c["N"], c["K"]) == 1
    _check(ops, _operands(c["M"], c["N"], c["K"], c["rps"], c["drop"], c["scale"], "int"), c["N"])
