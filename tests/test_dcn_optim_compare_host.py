"""Host-only checks of tests/dcn_cases.py and tests/optim_cases.py: the fp64 restatement of the deformable gather and its three gradients
agrees with oracle/dcn_ref.py run in fp64 (1e-11, on offsets of the 1/64 lattice where the fp32 coordinate addition is exact), the AdamW
restatement with optim.HFAdamW run in fp64, the ceilings of the calibrated constants are the numbers the kernels' operation counts give,
and seven local mutations that the older whole-tensor tolerances accept (rel-L2 1e-2 forward and optimizer, 2.5e-2 gradients) are
rejected by the per-element bounds with every constant AT ITS CEILING."""
import numpy as np
import pytest
import torch

from oracle import dcn_ref
from tests import dcn_cases as dc
from tests import optim_cases as oc
from tests.hip_util import assert_elementwise, rel_l2

T64 = lambda a: torch.from_numpy(np.array(a)).double()


def _rejected(name, got, ref, bound, tol):
    got, ref, bound = (T64(t).reshape(-1, t.shape[-1]) for t in (got, ref, np.broadcast_to(bound, ref.shape)))
    assert rel_l2(got, ref) <= tol, f"{name}: the mutation is not one that rel-L2 {tol} accepts ({rel_l2(got, ref):.3e})"
    assert not torch.equal(got, ref), f"{name}: the mutation changed nothing"
    with pytest.raises(AssertionError):
        assert_elementwise(name, got, ref, bound)


def _ceil(case, ref):
    return dc.ceilings(case, int(ref["dx_n"].max()))


# ---- the restatements against the oracles ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g_c8", "g_c24_s2", "s_c16_s1", "s_c32_s2", "t_one"])
def test_dcn_restatement_matches_the_oracle_in_fp64(name):
    case = dc.CASE_BY_NAME[name]
    inp = dc.make_inputs(case)
    assert np.array_equal(inp["offset"] * 64, np.round(inp["offset"] * 64)), "offsets off the 1/64 lattice"
    ref = dc.reference(case, inp)
    B, H, W, C, Ho, Wo, M, T = (case[k] for k in ("B", "H", "W", "C", "Ho", "Wo", "M", "T"))
    x = T64(inp["x"]).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    off = T64(inp["offset"]).view(B, Ho, Wo, 2 * T).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    msk = T64(inp["mask"]).view(B, Ho, Wo, T).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    cols = dcn_ref.sample_columns(x, off, msk, 3, 3, case["stride"], 1).permute(0, 3, 2, 1).reshape(M, T * C)     # [B, C, T, P] -> [M, T C]
    (cols * T64(inp["dcols"])).sum().backward()
    want = {"cols": cols.detach(), "dx": x.grad.permute(0, 2, 3, 1), "doffset": off.grad.permute(0, 2, 3, 1).reshape(M, 2 * T),
            "dmask": msk.grad.permute(0, 2, 3, 1).reshape(M, T)}
    for k, w in want.items():
        err = (T64(ref[k]) - w).abs() / w.abs().clamp_min(1.0)
        assert float(err.max()) <= 1e-11, (k, float(err.max()))
    # the ingredients the offset cases promise
    g = ref["geom"]
    h = dc.base_coords(case)[0] + inp["offset"][:, 0::2].astype(np.float64)
    assert (h == -1).any() and (h == H).any() and ((h > -1) & (h < 0)).any() and ((h > H - 1) & (h < H)).any() and (h == H - 1).any()
    assert (g["inn"] & (g["lh"] == 0) & (g["lw"] == 0)).any()


def test_tiled_cases_hold_what_they_promise():
    far = dc.reference(dc.CASE_BY_NAME["t_far"], dc.make_inputs(dc.CASE_BY_NAME["t_far"]))
    assert far["n_far"].sum() > 500 and far["straddle"] > 50 and np.abs(dc.make_inputs(dc.CASE_BY_NAME["t_far"])["offset"]).max() <= 7
    assert bool(far["geom"]["inn"].all())
    for name in ("t_plain",):
        assert dc.reference(dc.CASE_BY_NAME[name], dc.make_inputs(dc.CASE_BY_NAME[name]))["n_far"].sum() == 0
    for name, e in (("t_max_1", 1), ("t_max_below_1", 0), ("t_max_2p120", 121), ("t_max_denormal", -126), ("t_pile", 1), ("t_zero", None)):
        assert dc.fixed_exponent(dc.make_inputs(dc.CASE_BY_NAME[name])["dcols"]) == e, name
    for name, n in (("t_pile", 2304), ("t_pile4", 4 * 2304)):
        r = dc.reference(dc.CASE_BY_NAME[name], dc.make_inputs(dc.CASE_BY_NAME[name]))
        assert r["dx_n"].max() == n == r["n_win"].max() and np.count_nonzero(r["dx"]) == 16
        assert np.all(r["dx"][r["dx"] != 0] == n * dc.PILE_VALUE)
    assert 4 * 2304 * dc.PILE_VALUE * 2.0 ** 18 > 2 ** 31 > 2304 * dc.PILE_VALUE * 2.0 ** 18
    seams = dc.CASE_BY_NAME["t_seams"]
    assert dc.tiling(seams) == (16, 3, 3) and dc.tiling(dc.CASE_BY_NAME["t_s2"]) == (8, 2, 3)
    assert {dc.scatter_group(C) for C in dc.SCATTER_C} == {1, 2, 4, 8, 16, 32, 64}


def test_adam_restatement_matches_hfadamw_in_fp64():
    """betas whose complements are exact in fp32, so that the two differ only by the fp32 rounding of step_size"""
    from fiber_amd.optim import HFAdamW
    for base in oc.ADAM_CASES:
        case = dict(base, b1=0.875, b2=0.96875)
        lr, wd, b1, b2, eps, ss = oc.hyper_scalars(case)
        for st in oc.make_state(case)[3:8]:
            p = torch.nn.Parameter(T64(st["p"]))
            p.grad = T64(st["g"])
            opt = HFAdamW([p], lr=float(lr), betas=(float(b1), float(b2)), eps=float(eps), weight_decay=float(wd))
            opt.state[p].update(step=case["step"] - 1, exp_avg=T64(st["m"]).clone(), exp_avg_sq=T64(st["v"]).clone())
            opt.step()
            m1, v1, _, _ = oc.moments_reference(case, st)
            p1, term = oc.param_reference(case, st["p"], m1, v1)
            assert float((T64(m1) - opt.state[p]["exp_avg"]).abs().max()) <= 1e-13 * float(np.abs(m1).max())
            assert float((T64(v1) - opt.state[p]["exp_avg_sq"]).abs().max()) <= 1e-13 * float(np.abs(v1).max())
            moved = T64(term - np.abs(st["p"].astype(np.float64)))     # |update| + |decay|: what the fp32 rounding of step_size scales
            assert bool(((T64(p1) - p.detach()).abs() <= 2.0 ** -23 * moved + 1e-14).all())


def test_ceilings_are_the_operation_counts():
    by = dc.CASE_BY_NAME
    assert dc.ceilings(by["s_c8_s1"], 39) == {"CORNER": 16.0, "CH": 34.0, "DX": 88.0}
    assert dc.ceilings(by["s_c24_s1"])["CH"] == 52.0 and dc.ceilings(by["s_c512_s1"])["CH"] == 46.0 and dc.ceilings(by["s_c520_s1"])["CH"] == 62.0
    assert oc.CEILING == {"M": 6.0, "V": 8.0, "P": 16.0}
    for case in dc.CASES:
        top = dc.ceilings(case, 16)                           # 16: the busiest pixel of the smallest scatter geometry
        assert all(dc.CONST[k] <= top[k] for k in dc.CONST), (case["name"], top)
    assert all(oc.CONST[k] <= oc.CEILING[k] for k in oc.CONST)


def test_bf16_bits_round_to_nearest_even():
    a = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -0.0, np.inf, 2.0 ** -134, 3 * 2.0 ** -134, 1.0], np.float32)
    assert [hex(v) for v in oc.bf16_bits(a)] == ["0x3f80", "0x3f82", "0x8000", "0x7f80", "0x0", "0x2", "0x3f80"]
    r = torch.randn(4096).numpy()
    assert np.array_equal(oc.bf16_bits(r), torch.from_numpy(r).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


# ---- mutations -----------------------------------------------------------------------------------------------------------------------------
LIKE_TILED = dc._case("like_25x38", "tiled", 1, 25, 38, 16, 1, off="randn")
LIKE_13x17 = dc._case("like_13x17", "scatter", 2, 13, 17, 64, 1, off="randn")
# a wide strip: the border column is 1 / 768 of the map (on the 13 x 17 map it is 1 / 17 and rel-L2 reads 0.12: there the norm does notice)
LIKE_WIDE = dc._case("like_5x768", "scatter", 1, 5, 768, 8, 1, off="randn")


def _far_case():
    """random sigma = 1.2 offsets as in test_hip_dcn.py, three of them 5 px: past the halo"""
    inp = dc.make_inputs(LIKE_TILED)
    for m, t in ((40, 0), (500, 17), (900, 4)):
        inp["offset"][m, t] = 5.0 if t % 2 else -5.0
    return inp


def test_dropped_far_contributions_are_rejected():
    inp = _far_case()
    ref = dc.reference(LIKE_TILED, inp)
    assert ref["n_far"].sum() > 0
    _rejected("far", ref["dx"] - ref["dx_far"], ref["dx"], dc.bounds(LIKE_TILED, ref, _ceil(LIKE_TILED, ref))["dx_tiled"], 2.5e-2)


def test_seam_row_counted_twice_is_rejected():
    inp = _far_case()
    ref = dc.reference(LIKE_TILED, inp, windows=True)
    got = ref["dx"].copy()
    y0 = x0 = -1 - dc.HALO                                     # window of tile (0, 0); its last row is map row 19, first row of nothing else
    y = y0 + dc.WIN - 1
    got[0, y, 0:x0 + dc.WIN] += ref["win"][0][dc.WIN - 1, -x0:]
    _rejected("seam", got, ref["dx"], dc.bounds(LIKE_TILED, ref, _ceil(LIKE_TILED, ref))["dx_tiled"], 2.5e-2)


def test_right_border_rule_off_by_one_is_rejected():
    inp = dc.make_inputs(LIKE_WIDE)
    ref, mut = dc.reference(LIKE_WIDE, inp), dc.reference(LIKE_WIDE, inp, mutate="border")
    b = dc.bounds(LIKE_WIDE, ref, _ceil(LIKE_WIDE, ref))
    _rejected("border dx", mut["dx"], ref["dx"], b["dx"], 2.5e-2)
    _rejected("border dmask", mut["dmask"], ref["dmask"], b["dmask"], 2.5e-2)


def test_zeroed_channel_group_of_one_tap_is_rejected():
    inp = dc.make_inputs(LIKE_13x17)
    ref = dc.reference(LIKE_13x17, inp, grads=False)
    got = ref["cols"].copy()
    C = LIKE_13x17["C"]
    got[200, 4 * C + 8:4 * C + 16] = 0
    _rejected("group", got, ref["cols"], dc.bounds(LIKE_13x17, ref, dc.ceilings(LIKE_13x17))["cols"], 1e-2)


def test_left_derivative_on_integer_samples_is_rejected():
    inp = dc.make_inputs(LIKE_13x17)
    inp["offset"][5, 8], inp["offset"][200, 9] = 1.0, -1.0       # two samples exactly on an integer row / column
    ref, mut = dc.reference(LIKE_13x17, inp), dc.reference(LIKE_13x17, inp, mutate="left")
    assert np.allclose(mut["cols"], ref["cols"], rtol=0, atol=1e-12)
    _rejected("left", mut["doffset"], ref["doffset"], dc.bounds(LIKE_13x17, ref, _ceil(LIKE_13x17, ref))["doffset"], 2.5e-2)


def _adam_host(case, i):
    st = oc.make_state(case)[i]
    m1, v1, tm, tv = oc.moments_reference(case, st)
    p1, tp = oc.param_reference(case, st["p"], m1, v1)
    return st, m1, v1, p1, tp


def test_adam_tail_not_updated_is_rejected():
    case = oc.ADAM_BY_NAME["step1000_wd0"]
    st, m1, v1, p1, tp = _adam_host(case, 10)                   # n = 4099: n % 4 = 3
    got = p1.copy()
    got[-3:-1] = st["p"][-3:-1]                                 # (the last element holds the 1e15 gradient)
    _rejected("tail", got[:, None], p1[:, None], (oc.CEILING["P"] * oc.F32 * tp + oc.TINY32)[:, None], 1e-2)


def test_bf16_copy_lagging_one_step_is_rejected():
    case = oc.ADAM_BY_NAME["step1"]
    st, m1, v1, p1, tp = _adam_host(case, 8)
    new, old = oc.bf16_bits(p1.astype(np.float32)), oc.bf16_bits(st["p"])
    f = lambda b: (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    assert rel_l2(T64(f(old)), T64(f(new))) <= 1e-2
    assert not np.array_equal(old, new), "a lagging copy must differ in its bits"
