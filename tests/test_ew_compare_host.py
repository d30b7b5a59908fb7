"""Host-only checks of tests/ew_cases.py: the hash restatement agrees with itself across the 8- and 4-element vector groupings the
kernels use, the DropPath draw stays below 2 at keep = 1, and four local mutations of element-wise / cross-entropy / embedding results
that a whole-tensor rel-L2 of 5e-3 (the tolerance of the older tests) accepts are rejected by the per-element bounds."""
import numpy as np
import pytest
import torch

from tests import ew_cases as ec
from tests.hip_util import assert_elementwise, rel_l2

REL = 5e-3
DROPPATH_TOP_SEED, DROPPATH_TOP_SAMPLE = 208044, 50


def _rejected(name, got, ref, bound):
    assert rel_l2(got, ref) <= REL, f"{name}: the mutation is not one that rel-L2 accepts"
    with pytest.raises(AssertionError):
        assert_elementwise(name, got, ref, bound)


@pytest.mark.parametrize("seed", [0, 0x5EED, (0xDEADBEEF << 32) | 17, (1 << 64) - 1])
def test_hash_groupings_agree(seed):
    """drop_keep_e(drop_base(s, b), e) == drop_keep(s, b + e): the 8-vector (stream_add, dropout), 4-vector (embedding) and per-element
    forms of the same flat index give the same mask, also for indices past 2^32 (vectors do not straddle it)."""
    for start in (0, 2 ** 32 - 4096, 3 * 2 ** 32 + 8):
        i = np.arange(start, start + 4096, dtype=np.uint64)
        t = ec.thresh_of(0.37)
        per_elem = ec.fmix32(ec.drop_base(seed, i)) >= np.uint32(t)
        m8 = ec.keep_mask(seed, start + 4096, 0.37, 8)[start:] if start == 0 else \
            ec.drop_keep_e(ec.drop_base(seed, i - i % np.uint64(8)), (i % np.uint64(8)).astype(np.uint32), t)
        m4 = ec.drop_keep_e(ec.drop_base(seed, i - i % np.uint64(4)), (i % np.uint64(4)).astype(np.uint32), t)
        assert np.array_equal(per_elem, m8) and np.array_equal(per_elem, m4)
        assert 0.55 < per_elem.mean() < 0.71


def test_hash_u32_matches_splitmix64():
    """hash_u32 is the splitmix64 finaliser of seed + idx * golden: pinned on two known values of the plain Python form"""
    def ref(seed, idx):
        z = (seed + idx * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & ((1 << 64) - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & ((1 << 64) - 1)
        return (z ^ (z >> 31)) >> 32
    for s in (0, 12345, (1 << 64) - 3):
        assert [int(v) for v in ec.hash_u32(s, np.arange(64))] == [ref(s, i) for i in range(64)]


def test_droppath_keep_one_is_one():
    """keep = 1: every factor is exactly 1.  A seed whose draw has h >= 2^32 - 128 (found by a host search) gave 2.0 under the old
    u = h 2^-32 draw, which rounds to 1.0f there."""
    seed, j = DROPPATH_TOP_SEED, DROPPATH_TOP_SAMPLE          # ec.seed_hitting_top(64) finds them (a linear host search, ~20 s)
    h = ec.hash_u32(seed, np.arange(64))
    assert h[j] >= np.uint32(2 ** 32 - 128)
    old = np.floor(np.float32(1.0) + h.astype(np.float32) * np.float32(1.0 / 4294967296.0)) / np.float32(1.0)
    assert old[j] == 2.0
    assert np.array_equal(ec.droppath_scale(64, 1.0, seed), np.ones(64, np.float32))
    s = ec.droppath_scale(1 << 16, 0.9, 7)
    assert set(np.unique(s).tolist()) == {0.0, float(np.float32(1) / np.float32(0.9))}


def test_ce_head_with_another_rows_lse_is_rejected():
    g = torch.Generator().manual_seed(1)
    rows, V = 64, 50265
    x = (torch.randn(rows, V, generator=g) * 2).to(torch.bfloat16)
    lab = torch.randint(0, V, (rows,), generator=g)
    lse, _, _, _ = ec.ce_ref(x, lab, -100)
    ref, p = ec.ce_bwd_ref(x, lab, lse, 1.0 / rows, -100)
    got = ref.clone()
    r = 5
    head = (8 - (r * V) % 8) % 8
    got[r, :head] = (torch.exp(x[r, :head].double() - lse[r + 1]) - 0) / rows
    bound = ec.BF16_STORE * ref.abs() + ec.EXP_FLOOR / rows + ec.CONST["EXP"] * p * (1 + x.double().abs() + lse.abs()[:, None]) / rows
    assert head > 0
    _rejected("ce head", got, ref, bound)


def test_dropped_last_colsum_slab_is_rejected():
    g = torch.Generator().manual_seed(2)
    M, N = 300001, 128
    x = (torch.rand(M, N, generator=g) + 0.5).to(torch.bfloat16)
    ref, term = ec.colsum_ref(x)
    slabs = 512
    rpb = -(-M // slabs)
    got = x[: (slabs - 1) * rpb].double().sum(0)
    _rejected("colsum", got[:, None], ref[:, None], (ec.CONST["SUM"] * term)[:, None])


def test_missing_dpos_row_is_rejected():
    g = torch.Generator().manual_seed(3)
    B, S, C, pad = 4096, 40, 32, 1
    ids = torch.randint(3, 1000, (B, S), generator=g)
    for b in range(B):
        ids[b, 8 + b % 30:] = pad                            # ragged lengths: the last positions are rare
    ids[0, :] = torch.randint(3, 1000, (S,), generator=g)
    word, pos_tab, type_tab = torch.randn(1000, C, generator=g), torch.randn(S + 2, C, generator=g), torch.randn(1, C, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    f = ec.embed_fwd_ref(ids, word, pos_tab, type_tab, gamma, beta, pad, 1e-5)
    dy = torch.randn(B, S, C, generator=g).to(torch.bfloat16)
    out = ec.embed_bwd_ref(ids, f["pos"], dy, gamma, f["x"], f["mean"], f["rstd"], 1000, S + 2, pad)
    ref, term = out["dpos"]
    got = ref.clone()
    got[S + 1] = 0                                            # the last position: only sample 0 reaches it
    _rejected("dpos", got, ref, ec.CONST["EMB"] * term)


def test_one_vector_with_the_other_branchs_mask_is_rejected():
    g = torch.Generator().manual_seed(4)
    n = 1 << 16
    a, b = torch.randn(n, generator=g).to(torch.bfloat16), torch.randn(n, generator=g).to(torch.bfloat16)
    res = torch.randn(n, generator=g).to(torch.bfloat16)
    ref, term = ec.stream_add_ref(res, a, b, 0.5, None, 0.1, 11, 0.1, 12)
    ma, mb = ec.mask_t(11, n, 0.1, "cpu"), ec.mask_t(12, n, 0.1, "cpu")
    assert not torch.equal(ma[800:808], mb[800:808])
    got = ref.clone()
    ma2 = ma.clone()
    ma2[800:808] = mb[800:808]
    va = torch.where(ma2, a.double() * ec.inv_keep(0.1), torch.zeros(n, dtype=torch.float64))
    vb = torch.where(mb, b.double() * ec.inv_keep(0.1), torch.zeros(n, dtype=torch.float64))
    got[800:808] = (res.double() + va + 0.5 * vb)[800:808]
    _rejected("stream_add", got[:, None], ref[:, None], (ec.BF16_STORE * ref.abs() + ec.CONST["EW"] * term)[:, None])
