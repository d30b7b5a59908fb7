"""The autograd layer of fiber_amd/ops.py against fp64 under graph variants (tests/autograd_cases.py is the table):
  (a) every input live -- the baseline, which also reports the constant each family needs
  (b) frozen subsets: frozen inputs get no gradient, live ones stay inside the bound of (a), the forward output is bitwise that of (a)
  (c) forms of the incoming gradient (stride 0, transposed storage, a 2-byte offset): bitwise the aligned run
  (d) an intermediate with a second consumer, created before and after the first: the hand-over slots must not be believed
  (e) outputs of multi-output Functions that never reach the loss
  (f) the backward twice on a retained graph: bitwise equal, no slot left armed
  (g) a stale labelled-rows offer matched by a later pass
  (h) more rows than the labelled-rows column sum holds
Both hand-over slots are empty after every test of this file."""
import pytest
import torch

from tests import autograd_cases as AC
from tests.hip_util import DEV, assert_elementwise, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from fiber_amd import ops as ops_mod
    return ops_mod


@pytest.fixture(autouse=True)
def _slots_empty(ops):
    yield
    assert getattr(ops._rows_tls, "slot", None) is None, "labelled-rows slot left armed"
    assert getattr(ops._hint_tls, "slot", None) is None, "column-sum slot left armed"


def _run(ops, entry, live, gs=None, mid=AC.plain_mid):
    """(outputs, {leaf: grad}) of one forward + backward on fresh leaves"""
    case = entry.case(DEV)
    L = AC.leaves_of(case, live)
    outs = entry.run(ops, L, case.extra, mid)
    AC.backward(outs, case.gs if gs is None else gs)
    return outs, {k: L[k].grad for k in L}, L


def _check(entry, tag, got, G, B):
    worst = {}
    for k, g in G.items():
        if g is None:
            assert got[k] is None, f"{entry.name} {tag}: frozen {k} received a gradient"
        else:
            assert got[k] is not None, f"{entry.name} {tag}: live {k} received no gradient"
            worst[k] = assert_elementwise(f"{entry.name} {tag} d{k}", got[k].reshape(g.shape), g, B[k])
    return worst


_fwd = {}


def _baseline(ops, entry):
    """forward outputs of the all-live run, computed once per entry"""
    if entry.name not in _fwd:
        outs, _, _ = _run(ops, entry, tuple(entry.case(DEV).leaves))
        _fwd[entry.name] = [o.detach().clone() if o is not None else None for o in outs]
    return _fwd[entry.name]


def _same_forward(ops, entry, outs, tag):
    for i, (o, b) in enumerate(zip(outs, _baseline(ops, entry))):
        if o is not None and b is not None:
            assert torch.equal(o.detach(), b), f"{entry.name} {tag}: forward output {i} differs from the all-live run"


# ---- (a), (b): fp64 autograd entries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", AC.AUTOGRAD, ids=repr)
def test_all_live(ops, entry):
    case = entry.case(DEV)
    live = tuple(case.leaves)
    outs, got, _ = _run(ops, entry, live)
    G, B, A = AC.reference(entry, case, live, case.gs)
    L64 = AC.leaves_of(case, (), torch.float64)
    for o, r in zip(outs, entry.ref(L64, case.extra)):
        if o is not None and r is not None:
            assert rel_l2(o, r) < 1e-2, f"{entry.name}: forward"
    for k in G:
        need = AC.needed(got[k].reshape(G[k].shape), G[k], A[k])
        print(f"CALIB {entry.fam(k)} {entry.name} d{k}: needed {need:.3e} (CONST {AC.CONST[entry.fam(k)]:.3e})")
    _check(entry, "(a)", got, G, B)


@pytest.mark.parametrize("entry", AC.AUTOGRAD, ids=repr)
def test_frozen_subsets(ops, entry):
    case = entry.case(DEV)
    for live in AC.subsets(case):
        outs, got, _ = _run(ops, entry, live)
        _same_forward(ops, entry, outs, f"(b) live={live}")
        G, B, _ = AC.reference(entry, case, live, case.gs)
        assert [k for k in G if G[k] is not None] == [k for k in case.leaves if k in live]
        _check(entry, f"(b) live={live}", got, G, B)


# ---- (a), (b), (d) for the projection under window attention ------------------------------------------------------------------------
WIN = [e for e in AC.ENTRIES if e.family == "win_linear"]


def _manual_check(entry, tag, got, live, G, Bd):
    for k in entry.case(DEV).leaves:
        if k not in live:
            assert got[k] is None, f"{entry.name} {tag}: frozen {k} received a gradient"
        else:
            assert_elementwise(f"{entry.name} {tag} d{k}", got[k], G[k], Bd[k])


@pytest.mark.parametrize("colsum", [False, True], ids=["wgrad-sums", "win-colsum"])
@pytest.mark.parametrize("entry", WIN, ids=repr)
def test_window_projection_all_live_and_frozen(ops, entry, colsum):
    case = entry.case(DEV)
    names = tuple(case.leaves)
    was = ops._WIN_COLSUM
    ops._WIN_COLSUM = colsum
    try:
        base = None
        for live in [names] + AC.subsets(case):
            outs, got, L = _run(ops, entry, live)
            if base is None:
                base = outs[0].detach().clone()
            assert torch.equal(outs[0].detach(), base), f"{entry.name} live={live}: forward differs from the all-live run"
            if not outs[0].requires_grad:
                continue
            G, Bd, A = entry.grads({k: v.detach() for k, v in L.items()}, case.extra, case.gs, qkv=case.extra["qkv_seen"])
            if live == names:
                for k in ("x", "w", "b"):
                    need = AC.needed(got[k], G[k], A[k])
                    print(f"CALIB win_linear {entry.name} colsum={colsum} d{k}: needed {need:.3e} (CONST {AC.CONST['win_linear']:.3e})")
            _manual_check(entry, f"colsum={colsum} live={live}", got, live, G, Bd)
    finally:
        ops._WIN_COLSUM = was


@pytest.mark.parametrize("entry", [e for e in AC.MANUAL if e.family == "mha"], ids=repr)
def test_attention_all_live_and_frozen(ops, entry):
    case = entry.case(DEV)
    names = tuple(case.leaves)
    base = None
    for live in [names] + AC.subsets(case):
        outs, got, L = _run(ops, entry, live)
        if base is None:
            base = outs[0].detach().clone()
        assert torch.equal(outs[0].detach(), base), f"{entry.name} live={live}: forward differs from the all-live run"
        G, Bd, _ = entry.grads({k: v.detach() for k, v in L.items()}, case.extra, case.gs)
        if live == names:
            for k in G:
                r = float(((got[k].double() - G[k]).abs() / Bd[k]).max())
                print(f"CALIB mha {entry.name} d{k}: {r:.3f} of the kernel-level bound")
        _manual_check(entry, f"live={live}", got, live, G, Bd)


# ---- (c): forms of the incoming gradient --------------------------------------------------------------------------------------------
def _forms(g):
    """{form: (tensor of that form, the same values fresh and aligned)}"""
    if g.dim() == 0:
        return {}
    if g.dim() == 1:                                         # a per-row gradient: one value expanded; every second element of a buffer
        ex = g[:1].clone().expand(g.shape)
        tr = torch.stack([g, g], 1)[:, 0]
    else:
        ex = g.reshape(-1, g.shape[-1])[0].clone().expand(g.shape)
        perm = tuple(reversed(range(g.dim())))
        tr = g.permute(perm).contiguous().permute(perm)
    buf = torch.empty(g.numel() + 1, dtype=g.dtype, device=g.device)
    off = buf[1:].view(g.shape)
    off.copy_(g)
    assert ex.stride(0) == 0 and not tr.is_contiguous() and off.is_contiguous() and off.data_ptr() % 16 == g.element_size()
    return {"stride0": (ex, ex.contiguous()), "transposed": (tr, g.clone()), "offset": (off, g.clone())}


@pytest.mark.parametrize("entry", [e for e in AC.ENTRIES if e.family != "lib" or "seq" in e.name], ids=repr)
def test_gradient_forms(ops, entry):
    case = entry.case(DEV)
    live = tuple(case.leaves)
    for form, (g, aligned) in _forms(case.gs[0]).items():
        _, want, _ = _run(ops, entry, live, [aligned] + case.gs[1:])
        _, got, _ = _run(ops, entry, live, [g] + case.gs[1:])
        for k in want:
            assert torch.equal(got[k], want[k]), f"{entry.name} (c) {form}: d{k} differs from the aligned run"


# ---- (d): an intermediate consumed twice ---------------------------------------------------------------------------------------------
class _Recorder:
    """Wraps an offer function of ops to record the address, version and shape of what was offered."""

    def __init__(self, ops, name):
        self.ops, self.name, self.real, self.seen = ops, name, getattr(ops, name), []

    def __enter__(self):
        def wrapped(t, *a):
            self.seen.append((t.data_ptr(), tuple(t.shape), t._version))
            return self.real(t, *a)
        setattr(self.ops, self.name, wrapped)
        return self

    def __exit__(self, *exc):
        setattr(self.ops, self.name, self.real)


def _two_consumers(aux_w, first, box):
    def mid(t, f):
        if first:
            a = (t * aux_w.to(t.dtype)).sum()
            y = f(t)
        else:
            y = f(t)
            a = (t * aux_w.to(t.dtype)).sum()
        t.register_hook(lambda g: box.append((g.data_ptr(), tuple(g.shape), g._version)))
        box.append(a)
        return y
    return mid


def _aux_weights(entry, shape):
    return AC._bf(shape, AC._gen(entry.name + "-aux"), DEV, 0.25)


@pytest.mark.parametrize("first", [True, False], ids=["aux-first", "aux-last"])
@pytest.mark.parametrize("entry", [e for e in AC.ENTRIES if e.family == "lib"], ids=repr)
def test_logits_consumed_twice(ops, entry, first):
    """loss = f(logits) + aux(logits): aux puts gradient on the rows f's backward left zero, so the decoder's bias gradient is the sum
    over ALL rows of the accumulated gradient, whichever of the two backward nodes ran first."""
    case = entry.case(DEV)
    live = tuple(case.leaves)
    rows, V = case.leaves["h"].shape[0], case.leaves["w"].shape[0]
    aux_w = _aux_weights(entry, (rows, V))
    box = []
    with _Recorder(ops, "_offer_labelled_rows") as rec:
        L = AC.leaves_of(case, live)
        outs = entry.run(ops, L, case.extra, _two_consumers(aux_w, first, box))
        a = box.pop(0)
        torch.autograd.backward([outs[0], a], [case.gs[0], torch.ones_like(a)])
    got = {k: L[k].grad for k in L}
    print(f"{entry.name} aux {'first' if first else 'last'}: offered {rec.seen}, accumulated gradient {box}; "
          f"address kept: {bool(rec.seen and box and rec.seen[0][0] == box[0][0])}")
    box64 = []
    L64 = AC.leaves_of(case, live, torch.float64)
    o64 = entry.ref(L64, case.extra, _two_consumers(aux_w.double(), first, box64))
    a64 = box64.pop(0)
    torch.autograd.backward([o64[0], a64], [case.gs[0].double(), torch.ones_like(a64)])
    A = entry.twin({k: v.detach() for k, v in L64.items()}, case.extra, case.gs, dmid=aux_w)
    G = {k: L64[k].grad for k in L64}
    _check(entry, "(d)", got, G, {k: AC.bound("lib", G[k], A[k]) for k in G})


@pytest.mark.parametrize("first", [True, False], ids=["aux-first", "aux-last"])
@pytest.mark.parametrize("entry", WIN, ids=repr)
def test_qkv_consumed_twice(ops, entry, first):
    """The same for the qkv projection under window attention with the attention backward's own column sums switched on."""
    case = entry.case(DEV)
    live = tuple(case.leaves)
    aux_w = _aux_weights(entry, case.leaves["x"].shape[:2] + (case.leaves["w"].shape[0],))
    box = []
    was = ops._WIN_COLSUM
    ops._WIN_COLSUM = True
    try:
        with _Recorder(ops, "_offer_colsum") as rec:
            L = AC.leaves_of(case, live)
            outs = entry.run(ops, L, case.extra, _two_consumers(aux_w, first, box))
            a = box.pop(0)
            torch.autograd.backward([outs[0], a], [case.gs[0], torch.ones_like(a)])
    finally:
        ops._WIN_COLSUM = was
    assert len(rec.seen) == 1
    got = {k: L[k].grad for k in L}
    print(f"{entry.name} aux {'first' if first else 'last'}: offered {rec.seen}, accumulated gradient {box}; "
          f"address kept: {bool(box and rec.seen[0][0] == box[0][0])}")
    G, Bd, _ = entry.grads({k: v.detach() for k, v in L.items()}, case.extra, case.gs, dmid=aux_w, qkv=case.extra["qkv_seen"])
    _manual_check(entry, "(d)", got, live, G, Bd)


@pytest.mark.parametrize("entry", [AC.BY_NAME[n] for n in ("packed", "packed-fork", "lnres", "lnres-x32")], ids=repr)
def test_output_consumed_twice(ops, entry):
    """The first output feeds two consumers: its gradient reaches the Function as autograd's fan-in sum of two parts."""
    case = entry.case(DEV)
    live = tuple(case.leaves)
    g0 = case.gs[0]
    part = (g0.float() * 0.5).to(BF)
    rest = (g0.float() - part.float()).to(BF)
    res = []
    for dt, run, L in ((None, lambda L: entry.run(ops, L, case.extra), AC.leaves_of(case, live)),
                       (torch.float64, lambda L: entry.ref(L, case.extra), AC.leaves_of(case, live, torch.float64))):
        outs = run(L)
        y = outs[0]
        c = lambda t: t if dt is None else t.to(dt)
        ys = [(y * 1.0), (y * 1.0)] + [o for o in outs[1:] if o is not None]
        torch.autograd.backward(ys, [c(part), c(rest)] + [c(g) for o, g in zip(outs[1:], case.gs[1:]) if o is not None])
        res.append({k: L[k].grad for k in L})
    gs = [part.double() + rest.double()] + case.gs[1:]
    A = entry.twin({k: v.double() for k, v in case.leaves.items()}, case.extra, gs)
    _check(entry, "(d)", res[0], res[1], {k: AC.bound(entry.fam(k), res[1][k], A[k]) for k in res[1]})


# ---- (e): unused outputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [0, 1], ids=["first-only", "second-only"])
@pytest.mark.parametrize("entry", [AC.BY_NAME[n] for n in ("lnres", "lnres-x32", "packed-fork")], ids=repr)
def test_unused_output(ops, entry, keep):
    case = entry.case(DEV)
    live = tuple(case.leaves)
    gs = [g if i == keep else None for i, g in enumerate(case.gs)]
    outs, got, _ = _run(ops, entry, live, gs)
    _same_forward(ops, entry, outs, "(e)")
    G, B, _ = AC.reference(entry, case, live, gs)
    for k in G:                                   # a leaf the kept output does not depend on: None in the reference, None or zeros here
        if G[k] is None and got[k] is not None:
            assert not bool(got[k].any()), f"{entry.name} (e): d{k} must be zero"
            got[k] = None
    _check(entry, f"(e) output {keep} only", got, G, B)


# ---- (f): the backward twice --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", AC.ENTRIES, ids=repr)
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
    for k in L:
        assert torch.equal(passes[0][k], passes[1][k]), f"{entry.name} (f): d{k} of the second pass differs"


# ---- (g): a stale offer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ce", "seq"])
def test_stale_labelled_rows_offer(ops, kind):
    """The loss on LEAF logits leaves its offer unanswered, and the leaf's .grad IS the offered tensor.  Written into and passed as the
    gradient of a lib_linear output of the same shape in a later pass, it must be summed over all its rows."""
    entry = AC.BY_NAME[f"lib-{kind}-37x24"]
    case = entry.case(DEV)
    lab = case.extra["lab"]
    rows, V = 37, 24
    g = AC._gen("stale-" + kind, DEV)
    logits = AC._bf((rows, V), g, DEV).requires_grad_(True)
    if kind == "ce":
        ops.cross_entropy(logits, lab, AC.IGNORE).backward()
        ignored = lab == AC.IGNORE
    else:
        ops.seq_logprob(logits, lab, AC.PAD).backward(case.gs[0])
        ignored = lab == AC.PAD
    armed = getattr(ops._rows_tls, "slot", None) is not None
    assert float(logits.grad[ignored].abs().max()) == 0.0 and int(ignored.sum()) > rows // 2
    logits.grad[ignored] += AC._bf((int(ignored.sum()), V), g, DEV)
    L = AC.leaves_of(case, ("b",))
    y = ops.lib_linear(L["h"], L["w"], L["b"])
    y.backward(gradient=logits.grad)
    want = logits.grad.double().sum(0)
    assert_elementwise(f"(g) {kind} db", L["b"].grad, want, AC.bound("lib", want, logits.grad.double().abs().sum(0)))
    assert not armed, "the offer outlived the backward pass it was made in"


# ---- (h): past the labelled-rows limit ------------------------------------------------------------------------------------------------
def test_labelled_rows_limit(ops):
    from fiber_amd import lib
    rows, V, K = 122881, 24, 48
    assert rows == lib.plain("fiber_colsum_labelled_max_rows") + 1
    g = AC._gen("limit", DEV)
    h, w, b = AC._bf((rows, K), g, DEV), AC._bf((V, K), g, DEV, 0.3).requires_grad_(True), AC._bf((V,), g, DEV, 0.1).requires_grad_(True)
    lab = torch.randint(0, V, (rows,), generator=g)
    lab[torch.rand(rows, generator=g) < 0.8] = AC.IGNORE
    lab = lab.to(DEV)
    logits = ops.lib_linear(h, w, b)
    seen = []
    logits.register_hook(lambda t: seen.append(t.detach()))
    ops.cross_entropy(logits, lab, AC.IGNORE).backward()
    dl = seen[0].double()
    assert_elementwise("(h) db", b.grad, dl.sum(0), AC.bound("lib", dl.sum(0), dl.abs().sum(0)))
    # one row fewer: the labelled-rows kernel serves the call
    real, launched = lib.call, []
    lib.call = lambda name, *a: (launched.append(name), real(name, *a))[1]
    try:
        b.grad = None
        ops.cross_entropy(ops.lib_linear(h[:-1], w, b), lab[:-1], AC.IGNORE).backward()
    finally:
        lib.call = real
    assert "fiber_colsum_labelled_bf16" in launched


def test_single_consumer_still_uses_both_hand_overs(ops):
    """The fixes may only cost a MISSED hand-over its separate pass: on the plain graphs both are still used."""
    from fiber_amd import lib
    real, launched = lib.call, []
    lib.call = lambda name, *a: (launched.append(name), real(name, *a))[1]
    was = ops._WIN_COLSUM
    ops._WIN_COLSUM = True
    try:
        for name in ("lib-ce-600x1000", "lib-seq-37x24"):
            launched.clear()
            _run(ops, AC.BY_NAME[name], tuple(AC.BY_NAME[name].case(DEV).leaves))
            assert "fiber_colsum_labelled_bf16" in launched, name
        for name in ("win-linear-s3", "win-hm-s0"):
            launched.clear()
            real_take, taken = ops._take_colsum, []
            ops._take_colsum = lambda t: (taken.append(real_take(t)), taken[-1])[1]
            try:
                _run(ops, AC.BY_NAME[name], tuple(AC.BY_NAME[name].case(DEV).leaves))
            finally:
                ops._take_colsum = real_take
            assert len(taken) == 1 and taken[0] is not None, name
            assert "fiber_colsum_bf16" not in launched
    finally:
        lib.call = real
        ops._WIN_COLSUM = was
