"""The table of tests/ground_autograd_cases.py on the host: every entry's reference formulas evaluated in fp32, with a bf16 rounding
where the Functions store bf16 (values forward, gradients backward), must sit inside the committed bounds around the fp64 reference;
the defects the graph tests exist for, planted into that evaluation, must leave the bound by at least 8x on some element, so that no
calibrated constant can be loose enough to hide them; the twins are positive wherever the reference gradient is not zero; and the
conditions under which the discrete decisions of a case (floor of a sampling coordinate, the clamp, the ATSS assignment, the kinks of
GIoU) are the same in fp32 and fp64 hold with a margin."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import atss_cases
import fpn_cases
import ground_cases
from tests import autograd_cases as AC
from tests import ground_autograd_cases as GC

BF = torch.bfloat16
DEVICE = "cpu"


def _emulate(entry, case, live, gs, mid=AC.plain_mid, extra=None):
    """{leaf: gradient} of the fp32 / bf16 emulation, rounded the way the Functions return it (bf16 leaves get bf16 gradients)"""
    E = case.extra if extra is None else extra
    if entry.ref is None:
        G, _, _ = entry.grads(AC.leaves_of(case, (), torch.float32), E, gs, live, dtype=torch.float32)
        return G
    L = AC.leaves_of(case, live, torch.float32)
    outs = entry.ref(L, E, mid, AC.rn_bf16)
    AC.backward(outs, gs, torch.float32)
    return {k: (L[k].grad.to(case.leaves[k].dtype) if L[k].grad is not None else None) for k in L}


def _ratio(got, ref, bound):
    return float(((got.double() - ref).abs() / bound).max())


def _violates(entry, leaf, defective, G, B, factor=8.0):
    r = _ratio(defective, G[leaf], B[leaf])
    assert r >= factor, f"{entry.name}: the planted defect in d{leaf} is only {r:.3g}x the bound"


@pytest.mark.parametrize("entry", GC.ENTRIES, ids=repr)
def test_fp32_evaluation_sits_inside_the_bounds(entry):
    case = entry.case(DEVICE)
    live = tuple(case.leaves)
    got = _emulate(entry, case, live, case.gs)
    G, B, A = GC.reference(entry, case, live, case.gs)
    for k in G:
        r = _ratio(got[k], G[k], B[k])
        assert r <= 1.0, f"{entry.name} d{k}: the fp32 evaluation is {r:.3g}x the bound"
        assert bool((A[k][G[k] != 0] > 0).all()), f"{entry.name} d{k}: the twin is zero where the gradient is not"


@pytest.mark.parametrize("entry", GC.ENTRIES, ids=repr)
def test_frozen_inputs_have_no_gradient_on_both_sides(entry):
    case = entry.case(DEVICE)
    for live in AC.subsets(case):
        got = _emulate(entry, case, live, case.gs)
        G, _, _ = GC.reference(entry, case, live, case.gs)
        assert [k for k in G if G[k] is not None] == [k for k in got if got[k] is not None] == [k for k in case.leaves if k in live]


def test_table_states_branch_and_atomics_of_every_entry():
    for e in GC.ENTRIES:
        assert e.branch and set(e.atomics) <= set(e.case(DEVICE).leaves), e.name
        assert e.fam(next(iter(e.case(DEVICE).leaves))) in GC.CONST


# ---- planted defects ------------------------------------------------------------------------------------------------------------------
def test_defect_bias_gradient_includes_the_padded_rows():
    """db taken from the wrong end of the 32 padded rows: the 5 zero rows in, the first 5 channels out"""
    entry = GC.BY_NAME["conv3-c16-27-f32"]
    case = entry.case(DEVICE)
    G, B, _ = GC.reference(entry, case, tuple(case.leaves), case.gs)
    _violates(entry, "b", F.pad(G["b"], (0, 5))[5:], G, B)
    dw = torch.cat([G["w"], torch.zeros(5, *G["w"].shape[1:], dtype=torch.float64)])[5:]
    _violates(entry, "w", dw, G, B)


def test_defect_dp_ignores_the_text_mask():
    entry = GC.BY_NAME["loss-bool-mask"]
    case = entry.case(DEVICE)
    live = tuple(case.leaves)
    G, B, _ = GC.reference(entry, case, live, case.gs)
    bad = _emulate(entry, case, live, case.gs, extra=dict(case.extra, mask=torch.ones_like(case.extra["mask"])))
    _violates(entry, "p", bad["p"], G, B)
    _violates(entry, "tbias", bad["tbias"], G, B)
    dead = case.extra["mask"] == 0
    assert int(dead.sum()) > 0 and not bool(G["p"][dead].any()) and not bool(G["tbias"][dead].any())


def test_defect_gradient_through_a_clamped_logit():
    entry = GC.BY_NAME["logits-clamp"]
    case = entry.case(DEVICE)
    live = tuple(case.leaves)
    G, B, _ = GC.reference(entry, case, live, case.gs)
    L = AC.leaves_of(case, live, torch.float64)
    GC._ground_s(L, AC.rn_none)[1].backward(case.gs[0].double())       # the unclamped logits (tbias gets no gradient from them)
    for k in ("x", "p", "log_scale"):
        _violates(entry, k, L[k].grad, G, B)
    margin = entry.clamped(AC.leaves_of(case, (), torch.float64))
    frac = float((margin > 0).double().mean())
    assert 0.1 < frac < 0.6, frac
    # fp32 rounds a logit of this size by up to 2^-24 * 2^16: the clamp decision of the kernel is the reference's
    assert float(margin.abs().min()) > 0.05, float(margin.abs().min())
    # a gradient on the clamped elements only reaches nothing
    only = torch.where(margin > 0, case.gs[0], torch.zeros(()))
    Gc, _, _ = GC.reference(entry, case, live, [only])
    assert all(not bool(Gc[k].any()) for k in Gc)


def test_defect_fan_in_drops_the_second_consumer():
    entry = GC.BY_NAME["dyconv"]
    case = entry.case(DEVICE)
    live = tuple(case.leaves)
    G, B, _ = GC.reference(entry, case, live, case.gs)
    bad = _emulate(entry, case, live, [case.gs[0], None])              # the offset tensor's gradient from the stride-1 conv alone
    for k in ("wo", "bo", "x"):
        _violates(entry, k, bad[k], G, B)
    # the fp32 offsets of the kernels are within 2^-20 of these: no coordinate may sit that close to an integer
    assert entry.coords(AC.leaves_of(case, (), torch.float64)) > 2.0 ** -12


def test_defect_d_lateral_omits_the_dropped_branch():
    for name, leaf in (("fpn-coarse-keep", "lateral"), ("fpn-coarse-keep", "coarse"), ("fpn-nocoarse-keep", "lateral"), ("fpn-ragged", "coarse")):
        entry = GC.BY_NAME[name]
        case = entry.case(DEVICE)
        live = tuple(case.leaves)
        G, B, _ = GC.reference(entry, case, live, case.gs)
        _violates(entry, leaf, _emulate(entry, case, live, [case.gs[0], None])[leaf], G, B)
    entry = GC.BY_NAME["fpn-chain"]                                    # the coarse level without what comes down from the fine one
    case = entry.case(DEVICE)
    G, B, _ = GC.reference(entry, case, tuple(case.leaves), case.gs)
    _violates(entry, "lat_c", _emulate(entry, case, tuple(case.leaves), [case.gs[0], None])["lat_c"], G, B)


def test_defect_giou_gradient_left_at_a_level_without_positives():
    entry = GC.BY_NAME["atss-level-empty"]
    case = entry.case(DEVICE)
    G, B, _ = GC.reference(entry, case, tuple(case.leaves), case.gs)
    assert not bool(G["reg2"].any()) and not bool(G["ctr2"].any()) and bool(G["reg0"].any())
    _violates(entry, "reg2", torch.full_like(G["reg2"], 2.0 ** -30), G, B)      # what an unwritten or stale buffer would hold
    _violates(entry, "ctr2", torch.full_like(G["ctr2"], 2.0 ** -30), G, B)
    live_entry = GC.BY_NAME["atss-all-levels"]
    Gl, _, _ = GC.reference(live_entry, live_entry.case(DEVICE), tuple(case.leaves), case.gs)
    _violates(entry, "reg2", Gl["reg2"], G, B)                         # ... or the gradient of a level that does have positives


# ---- the conditions of the cases ------------------------------------------------------------------------------------------------------
def test_atss_cases_do_what_their_names_say():
    want = {"atss-all-levels": (True, True, True), "atss-level-empty": (True, True, False), "atss-none": (False, False, False)}
    for entry in GC.ATSS:
        case = entry.case(DEVICE)
        pos = case.extra["labels"] > 0
        lo, per = 0, []
        for h, w in GC.ATSS_SIZES:
            per.append(bool(pos[:, lo:lo + h * w].any()))
            lo += h * w
        assert tuple(per) == want[entry.name], (entry.name, per)
        for k, v in case.extra["margins"].items():                     # the fp32 kernels take the decisions of the fp64 restatement
            assert v > atss_cases.MARGINS[k], (entry.name, k, v)
        _, _, r = entry.grads(AC.leaves_of(case, (), torch.float64), case.extra, case.gs, tuple(case.leaves))
        assert r["kink"] > atss_cases.MARGINS["kink"], (entry.name, r["kink"])
        if entry.name == "atss-none":
            assert not bool(r["sums"].any())


def test_nearest_rule_of_the_reference_is_the_kernels():
    for (H, W), (Hc, Wc) in (((6, 10), (3, 5)), ((7, 9), (4, 5))):
        idx = torch.arange(Hc * Wc, dtype=torch.float64).view(1, 1, Hc, Wc)
        up = F.interpolate(idx, size=(H, W), mode="nearest")[0, 0].long()
        ih, iw = fpn_cases.src_index(H, Hc), fpn_cases.src_index(W, Wc)
        assert np.array_equal(up.numpy(), ih[:, None] * Wc + iw[None, :])


def test_ground_reference_is_the_restatement_of_ground_cases():
    entry = GC.BY_NAME["loss-u8-mask"]
    case = entry.case(DEVICE)
    live = tuple(case.leaves)
    G, _, _ = GC.reference(entry, case, live, case.gs)
    L = case.leaves
    r = ground_cases.backward64(L["x"], L["p"], L["tbias"], L["log_scale"], case.extra["targets"], case.extra["mask"], 0.25, 2.0, g=0.75)
    for k, key in (("x", "dx"), ("p", "dp"), ("tbias", "dtbias")):
        assert float((G[k] - r[key]).abs().max()) <= 1e-12 * float(r[key].abs().max()), k
    assert abs(float(G["log_scale"]) - float(r["dlog_scale"])) <= 1e-12 * abs(float(r["dlog_scale"]))
