"""The per-element checker of tests/hip_util.py on the host.  A whole-tensor rel-L2 at the kernel tests' 5e-3 cannot see a wrong
row, an 8-column group, one tile or the ragged last tile of a 70001 x 1024 result; assert_elementwise must reject each of them and
still accept the bf16 rounding of the exact result and of an fp32 result with another summation order."""
import pytest
import torch

from tests.hip_util import abs_mm64, assert_close, assert_elementwise, mm64

M, N, K = 70001, 1024, 64
C_ACC = 2.0 ** -18                  # fp32 accumulation over K = 64 products: <= 64 * 2^-24 of sum |x_k w_k|


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(M, K, generator=g) + 0.5).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    ref = mm64(x, w)
    bound = 2.0 ** -8 * ref.abs() + C_ACC * abs_mm64(x, w)
    got = ref.to(torch.bfloat16)
    return x, w, ref, bound, got


def _ulp(v):
    """bf16 unit in the last place of each (non-zero) element of v"""
    return torch.exp2(torch.floor(torch.log2(v.abs().double())) - 7)


def _zero_row(got):
    got[12345] = 0


def _group_4ulp(got):
    g = got[4242, 520:528]
    got[4242, 520:528] = (g.double() + 4 * _ulp(g) * g.double().sign()).to(torch.bfloat16)


def _tile_scaled(got):
    t = got[256 * 100:256 * 101, 256:512]
    got[256 * 100:256 * 101, 256:512] = (t.double() * (1 + 2.0 ** -6)).to(torch.bfloat16)


def _ragged_last_tile(got):
    t = got[(M // 256) * 256:, 768:]                        # rows 69888..70000: 113 of the 256 rows of the last row tile
    got[(M // 256) * 256:, 768:] = (t.double() * (1 - 2.0 ** -6)).to(torch.bfloat16)


@pytest.mark.parametrize("mutate", [_zero_row, _group_4ulp, _tile_scaled, _ragged_last_tile], ids=lambda f: f.__name__[1:])
def test_elementwise_rejects_what_rel_l2_accepts(case, mutate):
    _, _, ref, bound, got = case
    bad = got.clone()
    mutate(bad)
    e = assert_close("mutated", bad, ref, 5e-3)              # the gap: the whole-tensor metric accepts the mutation ...
    with pytest.raises(AssertionError) as info:             # ... the per-element one does not
        assert_elementwise("mutated", bad, ref, bound)
    print(f"{mutate.__name__[1:]}: rel-L2 {e:.2e} accepted at 5e-3; assert_elementwise: {info.value}")


def test_elementwise_accepts_rounding_and_reordering(case):
    x, w, ref, bound, got = case
    r = assert_elementwise("bf16(exact)", got, ref, bound)
    assert r <= 1.0
    f32 = (x.float() @ w.float().t())                       # another summation order in fp32, then the bf16 store
    assert_elementwise("bf16(fp32 product)", f32.to(torch.bfloat16), ref, bound)
    assert_elementwise("fp32 product", f32, ref, C_ACC * abs_mm64(x, w))


def test_elementwise_reports_position_and_scalar_bounds():
    ref = torch.zeros(600, 40, dtype=torch.float64)
    got = ref.clone()
    got[513, 37] = 1.0
    got[2, 3] = 0.5
    with pytest.raises(AssertionError, match=r"2 of 24000 elements.*row 513, col 37\) = tile \(2, 0\)"):
        assert_elementwise("y", got, ref, 0.25)
    got[1, 1] = float("nan")
    with pytest.raises(AssertionError, match="3 of 24000"):
        assert_elementwise("y", got, ref, torch.full((40,), 0.25))
    assert_elementwise("y", ref, ref, 0.0)
