"""The bounds of tests/autograd_cases.py on the host: every entry's reference formulas evaluated in fp32, with a bf16 rounding where the
kernels store bf16 (values forward, gradients backward), must sit inside the committed bounds around the fp64 reference -- and the
defects the graph tests exist for, planted into that fp32 evaluation, must leave them by at least 8x on some element, so that no
calibrated constant can be loose enough to hide them."""
import pytest
import torch

from tests import autograd_cases as AC

BF = torch.bfloat16
DEVICE = "cpu"


def _emulate(entry, case, live, gs, mid=AC.plain_mid, extra=None):
    """{leaf: gradient} of the fp32 / bf16 emulation, rounded the way the Functions return it (bf16 leaves get bf16 gradients)"""
    L = AC.leaves_of(case, live, torch.float32)
    outs = entry.ref(L, case.extra if extra is None else extra, mid, AC.rn_bf16)
    AC.backward(outs, gs, torch.float32)
    return {k: (L[k].grad.to(case.leaves[k].dtype) if L[k].grad is not None else None) for k in L}


def _ratio(got, ref, bound):
    return float(((got.double() - ref).abs() / bound).max())


@pytest.mark.parametrize("entry", AC.HOST, ids=repr)
def test_fp32_evaluation_sits_inside_the_bounds(entry):
    case = entry.case(DEVICE)
    live = tuple(case.leaves)
    got = _emulate(entry, case, live, case.gs)
    G, B, _ = AC.reference(entry, case, live, case.gs)
    for k in G:
        r = _ratio(got[k], G[k], B[k])
        assert r <= 1.0, f"{entry.name} d{k}: the fp32 evaluation is {r:.3g}x the bound"


@pytest.mark.parametrize("entry", AC.HOST, ids=repr)
def test_frozen_inputs_have_no_gradient_on_both_sides(entry):
    case = entry.case(DEVICE)
    for live in AC.subsets(case):
        got = _emulate(entry, case, live, case.gs)
        G, _, _ = AC.reference(entry, case, live, case.gs)
        assert [k for k in G if G[k] is not None] == [k for k in got if got[k] is not None] == [k for k in case.leaves if k in live]


def _violates(entry, leaf, defective, G, B, factor=8.0):
    r = _ratio(defective, G[leaf], B[leaf])
    assert r >= factor, f"{entry.name}: the planted defect in d{leaf} is only {r:.3g}x the bound"


@pytest.mark.parametrize("name", ["lib-ce-37x24", "lib-ce-600x1000", "lib-seq-37x24", "lib-seq-600x1000"])
def test_defect_bias_gradient_over_labelled_rows_only(name):
    """db summed over the labelled rows while a second consumer of the logits wrote the other rows"""
    entry = AC.BY_NAME[name]
    case = entry.case(DEVICE)
    live = tuple(case.leaves)
    rows, V = case.leaves["h"].shape[0], case.leaves["w"].shape[0]
    aux_w = AC._bf((rows, V), AC._gen(name + "-aux"), DEVICE, 0.25)
    seen = []

    def mid(dtype):
        def m(t, f):
            a = (t * aux_w.to(dtype)).sum()
            t.register_hook(lambda g: seen.append(g.detach().clone()))
            return f(t), a
        return m

    L64 = AC.leaves_of(case, live, torch.float64)
    (y, a), = entry.ref(L64, case.extra, mid(torch.float64))
    torch.autograd.backward([y, a], [case.gs[0].double(), torch.ones_like(a)])
    A = entry.twin({k: v.detach() for k, v in L64.items()}, case.extra, case.gs, dmid=aux_w)
    G = {k: L64[k].grad for k in L64}
    B = {k: AC.bound("lib", G[k], A[k]) for k in G}
    seen.clear()
    L32 = AC.leaves_of(case, live, torch.float32)
    (y, a), = entry.ref(L32, case.extra, mid(torch.float32), AC.rn_bf16)
    torch.autograd.backward([y, a], [case.gs[0].float(), torch.ones_like(a)])
    for k in G:                                                    # the sound evaluation of the two-consumer graph is inside
        assert _ratio(L32[k].grad.to(BF), G[k], B[k]) <= 1.0, k
    dl = seen[0].to(BF).float()                                    # the accumulated gradient, as the fan-in add leaves it
    valid = case.extra["lab"] != (AC.IGNORE if "ce" in name else AC.PAD)
    _violates(entry, "b", dl[valid].sum(0).to(BF), G, B)


@pytest.mark.parametrize("name,leaves", [("linear-rs-fold", ("w", "b")), ("linear-rs-nofold", ("w", "b")), ("mlp64-rs-fold", ("w2", "b2", "w1")),
                                         ("mlp96-rs", ("w2", "w1"))])
def test_defect_droppath_factor_dropped_from_weight_gradient(name, leaves):
    entry = AC.BY_NAME[name]
    case = entry.case(DEVICE)
    live = tuple(case.leaves)
    G, B, _ = AC.reference(entry, case, live, case.gs)
    bad = _emulate(entry, case, live, case.gs, extra=dict(case.extra, rs=torch.ones_like(case.extra["rs"])))
    for k in leaves:
        _violates(entry, k, bad[k], G, B)


@pytest.mark.parametrize("name", ["linear-res", "linear-res32", "mlp64", "mlp96", "lnres", "lnres-x32", "stream-ab", "rowscale_add"])
def test_defect_residual_gradient_dropped(name):
    entry = AC.BY_NAME[name]
    case = entry.case(DEVICE)
    live = tuple(case.leaves)
    G, B, _ = AC.reference(entry, case, live, case.gs)
    if name.startswith("lnres"):                                   # the residual's gradient is added inside the LayerNorm backward
        bad = _emulate(entry, case, live, [case.gs[0], None])
        _violates(entry, "x", bad["x"], G, B)
    else:
        _violates(entry, "res", torch.zeros_like(G["res"]), G, B)


@pytest.mark.parametrize("name", ["scale_add", "stream-ab-alpha", "stream-ab-alpha-rs", "stream-res32"])
def test_defect_dalpha_omitted(name):
    entry = AC.BY_NAME[name]
    case = entry.case(DEVICE)
    G, B, _ = AC.reference(entry, case, tuple(case.leaves), case.gs)
    _violates(entry, "alpha", torch.zeros_like(G["alpha"]), G, B)


@pytest.mark.parametrize("name", ["lnmlp", "lnmlp-rs"])
def test_defect_ln_mlp_affine_gradients_from_unfolded_weights(name):
    """_LnMlp forms dgamma = colsum(dW1' * W1) and dbeta = W1^T db1 from the gradient of the FOLDED weight W1' = W1 diag(gamma): taking
    the unfolded dW1 = dW1' diag(gamma) + db1 (x) beta, or the folded weight, in their place is wrong by the factor gamma."""
    entry = AC.BY_NAME[name]
    case = entry.case(DEVICE)
    G, B, _ = AC.reference(entry, case, tuple(case.leaves), case.gs)
    w1, gamma = case.leaves["w1"].double(), case.leaves["gamma"].double()
    _violates(entry, "gamma", (G["w1"] * w1).sum(0), G, B)
    _violates(entry, "beta", (w1 * gamma[None, :]).t() @ G["b1"], G, B)


def test_defect_alias_gradient_dropped_from_forked_dx():
    entry = AC.BY_NAME["packed-fork"]
    case = entry.case(DEVICE)
    live = tuple(case.leaves)
    G, B, _ = AC.reference(entry, case, live, case.gs)
    bad = _emulate(entry, case, live, [case.gs[0], None])
    _violates(entry, "x", bad["x"], G, B)


def test_window_projection_reference_is_consistent_with_autograd():
    """The Function-by-Function fp64 gradients of the projection under window attention against fp64 autograd of the whole graph in the
    reference's formulation (roll, partition, softmax attention, reverse): the two must agree to the rounding of the bf16 qkv."""
    import torch.nn.functional as F
    for entry in [e for e in AC.ENTRIES if e.family == "win_linear"]:
        case = entry.case(DEVICE)
        c = entry.acase
        Bn, H, W, heads, ws, shift = (c[k] for k in ("B", "H", "W", "heads", "ws", "shift"))
        C = heads * 32
        L = AC.leaves_of(case, tuple(case.leaves), torch.float64)
        G, _, _ = entry.grads({k: v.detach() for k, v in L.items()}, case.extra, case.gs)
        qkv = F.linear(L["x"], L["w"], L["b"])
        tok, lab, rel = case.extra["tok"], case.extra["lab"], case.extra["rel"]
        u = qkv.view(-1, 3, heads, 32)[tok]                                         # [G, N, 3, heads, 32]
        q, k, v = (u[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        s = 32 ** -0.5 * q @ k.transpose(-1, -2) + L["table"][rel.reshape(-1)].view(ws * ws, ws * ws, heads).permute(2, 0, 1)[None]
        if shift:
            s = s + torch.where(lab[:, :, None] != lab[:, None, :], -100.0, 0.0).double()[:, None]
        o = (s.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(-1, C)
        out = torch.zeros(Bn * H * W, C, dtype=torch.float64).index_add(0, tok.reshape(-1), o)
        out.backward(case.gs[0].double().view(-1, C))
        for name in ("x", "w", "b", "table"):
            err = (L[name].grad - G[name]).abs().max() / G[name].abs().max()
            assert err < 2.0 ** -6, (entry.name, name, float(err))
