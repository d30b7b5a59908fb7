"""The grounding Functions of fiber_amd/ops.py (_DeformConv, _Conv1x1, _FpnMerge, _GroundLogits, _GroundTokenLoss, _AtssBoxLosses)
against fp64 under the graph variants of tests/test_hip_autograd_graphs.py (tests/ground_autograd_cases.py is the table):
  (a) every input live -- the baseline, which also reports the constant each family needs (CALIB lines)
  (b) frozen subsets: frozen inputs get no gradient, live ones stay inside the bound of (a), the forward output is bitwise that of (a)
  (c) forms of the incoming gradient (stride 0, transposed storage, a storage offset): bitwise the aligned run, within the bound where
      the path has fp32 atomics (entry.atomics)
  (d) an intermediate with a second consumer, created before and after the first (the offset tensor, `inner`, the logits), and a
      convolution output consumed twice
  (e) outputs that never reach the loss
  (f) the backward twice on a retained graph: bitwise equal (within the bound through atomics), no hand-over slot left armed"""
import itertools

import pytest
import torch

from tests import autograd_cases as AC
from tests import ground_autograd_cases as GC
from tests.hip_util import DEV, assert_elementwise, rel_l2
from tests.test_hip_autograd_graphs import _aux_weights, _check, _forms, _run, _same_forward, _slots_empty, _two_consumers, ops  # noqa: F401

pytestmark = pytest.mark.gpu


def _exact_zeros(entry, case, got, tag):
    for k, where in (entry.zeros(case) if entry.zeros else {}).items():
        if got.get(k) is not None:
            v = got[k][where.to(got[k].device)]
            assert not bool(v.isnan().any()) and not bool(v.any()), f"{entry.name} {tag}: d{k} must be exactly 0 where nothing is live"


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", GC.ENTRIES, ids=repr)
def test_all_live(ops, entry):
    case = entry.case(DEV)
    live = tuple(case.leaves)
    outs, got, _ = _run(ops, entry, live)
    G, B, A = GC.reference(entry, case, live, case.gs)
    if entry.ref is not None:
        for o, r in zip(outs, entry.ref(AC.leaves_of(case, (), torch.float64), case.extra)):
            if o is not None and r is not None:
                assert rel_l2(o, r) < 1e-2, f"{entry.name}: forward"
    else:
        a = case.extra["assignment"]
        assert torch.equal(a.labels, case.extra["labels"]), f"{entry.name}: the assignment is not the restatement's"
        _, _, r = entry.grads(AC.leaves_of(case, (), torch.float64), case.extra, case.gs, live)
        bound = GC.atss_cases.CONST["K_SUM"] * GC.atss_cases.EPS * r["sums_abs"]
        assert_elementwise(f"{entry.name} sums", torch.stack([o.detach() for o in outs]), r["sums"], bound)
    for k in G:
        need = AC.needed(got[k].reshape(G[k].shape), G[k], A[k])
        print(f"CALIB {entry.fam(k)} {entry.name} d{k}: needed {need:.3e} (CONST {GC.CONST[entry.fam(k)]:.3e})")
    _check(entry, "(a)", got, G, B)
    _exact_zeros(entry, case, got, "(a)")


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------
def _subsets(entry, case):
    """AC.subsets, and: only offset / mask live; one pyramid level frozen"""
    out = AC.subsets(case)
    names = list(case.leaves)
    extra = []
    if "offset" in names:
        extra.append(("offset", "mask"))
    if entry.family == "atss":
        extra += [tuple(n for n in names if n not in (f"reg{l}", f"ctr{l}")) for l in range(3)]
    return out + [s for s in extra if s not in out]


@pytest.mark.parametrize("entry", GC.ENTRIES, ids=repr)
def test_frozen_subsets(ops, entry):
    case = entry.case(DEV)
    for live in _subsets(entry, case):
        outs, got, _ = _run(ops, entry, live)
        _same_forward(ops, entry, outs, f"(b) live={live}")
        G, B, _ = GC.reference(entry, case, live, case.gs)
        assert [k for k in G if G[k] is not None] == [k for k in case.leaves if k in live]
        _check(entry, f"(b) live={live}", got, G, B)
        _exact_zeros(entry, case, got, f"(b) live={live}")


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------
def _same_or_bounded(entry, case, tag, got, want, gs):
    """bitwise `want` except through fp32 atomics, where both stay inside the bound"""
    live = tuple(case.leaves)
    if entry.atomics:
        G, B, _ = GC.reference(entry, case, live, gs)
    for k in want:
        if k in entry.atomics:
            for name, v in (("", got), (" (reference run)", want)):
                assert_elementwise(f"{entry.name} {tag} d{k}{name}", v[k].reshape(G[k].shape), G[k], B[k])
        else:
            assert torch.equal(got[k], want[k]), f"{entry.name} {tag}: d{k} differs"


@pytest.mark.parametrize("entry", [e for e in GC.AUTOGRAD if e.name not in ("loss-u8", "loss-bool-mask", "loss-u8-mask")], ids=repr)
def test_gradient_forms(ops, entry):
    case = entry.case(DEV)
    live = tuple(case.leaves)
    forms = _forms(case.gs[0])
    assert len(forms) == 3
    for form, (g, aligned) in forms.items():
        _, want, _ = _run(ops, entry, live, [aligned] + case.gs[1:])
        _, got, _ = _run(ops, entry, live, [g] + case.gs[1:])
        _same_or_bounded(entry, case, f"(c) {form}", got, want, [aligned] + case.gs[1:])


@pytest.mark.parametrize("entry", GC.ATSS, ids=repr)
def test_gradient_forms_of_the_three_sums(ops, entry):
    """the [3] gradient of the sums as an expanded scalar, strided and offset: read from device memory through `_c(g.float().reshape(3))`"""
    case = entry.case(DEV)
    live = tuple(case.leaves)
    for form, (g, aligned) in _forms(torch.stack(case.gs)).items():
        res = []
        for g3 in (aligned, g):
            L = AC.leaves_of(case, live)
            entry.run_sums(ops, L, case.extra).backward(g3)
            res.append({k: L[k].grad for k in L})
        for k in res[0]:
            assert torch.equal(res[0][k], res[1][k]), f"{entry.name} (c) {form}: d{k} differs from the aligned run"
        G, B, _ = GC.reference(entry, case, live, list(aligned))
        _check(entry, f"(c) {form}", res[1], G, B)


# ---- (d) ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [True, False], ids=["aux-first", "aux-last"])
@pytest.mark.parametrize("entry", [e for e in GC.ENTRIES if e.mid_shape], ids=repr)
def test_intermediate_consumed_twice(ops, entry, first):
    """loss = f(t) + aux(t) for the offset tensor, the coarse `inner` and the logits: the Function that made t receives autograd's
    fan-in sum, whichever consumer was created first"""
    case = entry.case(DEV)
    live = tuple(case.leaves)
    aux_w = _aux_weights(entry, entry.mid_shape)
    res = []
    for dt, fn in ((None, lambda L, m: entry.run(ops, L, case.extra, m)), (torch.float64, lambda L, m: entry.ref(L, case.extra, m))):
        box = []
        L = AC.leaves_of(case, live, dt)
        outs = fn(L, _two_consumers(aux_w if dt is None else aux_w.to(dt), first, box))
        a = box.pop(0)
        c = (lambda t: t) if dt is None else (lambda t: t.to(dt))
        torch.autograd.backward(list(outs) + [a], [c(g) for g in case.gs] + [torch.ones_like(a)])
        res.append({k: L[k].grad for k in L})
    A = entry.twin({k: v.double() for k, v in case.leaves.items()}, case.extra, case.gs, dmid=aux_w)
    _check(entry, "(d)", res[0], res[1], {k: AC.bound(entry.fam(k), res[1][k], A[k]) for k in res[1]})


@pytest.mark.parametrize("entry", [GC.BY_NAME[n] for n in ("dcn-c16-s1", "dcn-c8", "conv3-c16-bias", "conv3-c16-27-f32", "conv1x1-bias",
                                                           "fpn-coarse-keep", "logits")], ids=repr)
def test_output_consumed_twice(ops, entry):
    """The first output feeds two consumers: its gradient reaches the Function as autograd's fan-in sum of two parts (which add up to
    the gradient of the table exactly, so the bound of (a) holds unchanged)."""
    case = entry.case(DEV)
    live = tuple(case.leaves)
    g0 = case.gs[0]
    part = (g0.float() * 0.5).to(g0.dtype)
    rest = (g0.float() - part.float()).to(g0.dtype)
    assert torch.equal((part.double() + rest.double()).to(g0.dtype), g0)
    L = AC.leaves_of(case, live)
    outs = entry.run(ops, L, case.extra)
    ys = [outs[0] * 1.0, outs[0] * 1.0] + [o for o in outs[1:] if o is not None]
    torch.autograd.backward(ys, [part, rest] + [g for o, g in zip(outs[1:], case.gs[1:]) if o is not None])
    G, B, _ = GC.reference(entry, case, live, case.gs)
    _check(entry, "(d)", {k: L[k].grad for k in L}, G, B)


# ---- (e) ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", [GC.BY_NAME[n] for n in ("dyconv", "fpn-coarse-keep", "fpn-nocoarse-keep", "fpn-ragged", "fpn-chain")] + GC.ATSS, ids=repr)
def test_unused_outputs(ops, entry):
    """every proper subset of the outputs reaching the loss, the empty one included; for the ATSS sums also a gradient of zeros for sum w"""
    case = entry.case(DEV)
    live = tuple(case.leaves)
    n = len(case.gs)
    variants = [[g if i in keep else None for i, g in enumerate(case.gs)] for r in range(n) for keep in itertools.combinations(range(n), r)]
    if entry.family == "atss":
        variants.append([case.gs[0], torch.zeros_like(case.gs[1]), case.gs[2]])
    for gs in variants:
        tag = f"(e) outputs {[i for i, g in enumerate(gs) if g is not None]}"
        outs, got, _ = _run(ops, entry, live, gs)
        _same_forward(ops, entry, outs, tag)
        G, B, _ = GC.reference(entry, case, live, gs)
        for k in G:                               # a leaf the kept outputs do not depend on: None in the reference, None or zeros here
            if G[k] is None and got[k] is not None:
                assert not bool(got[k].any()), f"{entry.name} {tag}: d{k} must be zero"
                got[k] = None
        _check(entry, tag, got, G, B)
        _exact_zeros(entry, case, got, tag)


# ---- (f) ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", GC.ENTRIES, ids=repr)
def test_backward_twice(ops, entry):
    case = entry.case(DEV)
    L = AC.leaves_of(case, tuple(case.leaves))
    outs = entry.run(ops, L, case.extra)
    passes = []
    for i in range(2):
        pairs = [(y, g) for y, g in zip(outs, case.gs) if y is not None]
        torch.autograd.backward([p[0] for p in pairs], [p[1] for p in pairs], retain_graph=True)
        assert getattr(ops._rows_tls, "slot", None) is None and getattr(ops._hint_tls, "slot", None) is None, f"slot armed after pass {i}"
        passes.append({k: L[k].grad.clone() for k in L})
        for k in L:
            L[k].grad = None
    _same_or_bounded(entry, case, "(f) second pass", passes[1], passes[0], case.gs)


# ---- the exact zeros of the clamp and of an empty anchor set ----------------------------------------------------------------------------
def test_gradient_on_clamped_logits_only_reaches_nothing(ops):
    entry = GC.BY_NAME["logits-clamp"]
    case = entry.case(DEV)
    live = tuple(case.leaves)
    L = AC.leaves_of(case, live)
    (out,) = entry.run(ops, L, case.extra)
    clamped = out.detach().abs() >= 50000.0
    assert 0.1 < float(clamped.float().mean()) < 0.6
    assert torch.equal(clamped, entry.clamped(AC.leaves_of(case, (), torch.float64)) > 0), "the kernel clamps other elements than the reference"
    out.backward(torch.where(clamped, case.gs[0], torch.zeros((), device=DEV)))
    for k in L:
        assert L[k].grad is not None and not bool(L[k].grad.any()), f"d{k} through clamped logits must be exactly 0"


def test_token_loss_without_anchors_is_a_constant(ops):
    entry = GC.BY_NAME["loss-u8"]
    case = entry.case(DEV)
    L = AC.leaves_of(case, tuple(case.leaves))
    x0 = L["x"][:, :0]
    loss = ops.ground_token_loss(x0, L["p"], L["tbias"], L["log_scale"], case.extra["targets"][:, :0], None)
    assert loss.shape == () and float(loss) == 0.0 and not loss.requires_grad
    (loss + (L["tbias"] * 0).sum()).backward()                         # the constant takes part in a graph without touching the leaves
    assert all(L[k].grad is None for k in ("x", "p", "log_scale")) and not bool(L["tbias"].grad.any())
