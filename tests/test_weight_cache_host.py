"""Host: the derived weight copies of fiber_amd/ops.py follow their fp32 masters through every way a parameter changes
(tests/weight_cache_cases.py has the expected values, the audit, the cases and the writers).  The kinds whose accessors are
plain torch run here, which is all of them: plain, transposed, head-major qkv, packs, the LayerNorm-folded Mlp
set, the patch embedding, conv rows and their transpose, the 2-D view of a 1x1 conv.  The consuming ops are HIP
kernels, so here "the op" is its accessor calls; tests/test_hip_weight_cache.py runs the ops."""
import pytest
import torch

import weight_cache_cases as wc
from fiber_amd import ops


@pytest.fixture(autouse=True)
def _fresh_cache():
    ops.clear_weight_cache()
    yield
    ops.clear_weight_cache()


def _entries(case):
    """(key, owner) of every entry the case's parameters have in the cache (a 1x1 conv's copies belong to its 2-D view)."""
    owners = {id(p): p for p in case.params}
    for k, v in list(ops._wcache.items()):
        if isinstance(k, tuple) and k[0] == "V2" and v[2]() is not None and id(v[2]()) in owners:
            owners[id(v[1])] = v[1]
    out = []
    for k, v in list(ops._wcache.items()):
        w = v[2]()
        if w is not None and id(w) in owners and not (isinstance(k, tuple) and k[0] == "V2"):
            out.append((k, w))
    return out


@pytest.mark.parametrize("writer", sorted(wc.HOST_WRITERS))
@pytest.mark.parametrize("name", wc.HOST_CASES)
def test_host_copies_follow_the_writer(name, writer):
    case = wc.make_cases("cpu", [name])[name]
    case.host()
    assert wc.audit(case.audit_args()) >= case.kinds, "the case did not create the copies it is about"
    before = _entries(case)
    assert before
    wc.HOST_WRITERS[writer](case)
    # no writer on the host rewrites a copy itself: each one must be stale by its own stamp now ...
    for key, w in before:
        ent = ops._cache_get(key, w)
        if ent is None:
            continue                                     # (gone with the view it belonged to: rebuilt from nothing)
        if isinstance(key, tuple) and key[0] == "HM":
            assert not wc.is_current(ops, key, w, case.groups[0].b), f"{name} / {writer}: HM entry still current"
        elif isinstance(key, tuple) and key[0] == "LNMLP":
            assert ent[0] != tuple(ops._stamp(t) for t in case.groups[0].five), f"{name} / {writer}: LNMLP entry still current"
        else:
            # (a copy that belongs to the 2-D view of a 1x1 conv is also out of use when the view no longer is the parameter's storage)
            orphan = name == "conv1x1" and w.data_ptr() != case.params[0].data_ptr()
            assert orphan or ent[0] != ops._stamp(w), f"{name} / {writer}: {key!r} still called current"
    assert not any(wc.pack_is_current(ops, s) for s in case.groups if isinstance(s, wc.Pack)), f"{name} / {writer}: pack still called current"
    # ... and the next accessor call must hand out the expected copy of the NEW master
    # (a 1x1 conv whose storage moved gets a NEW 2-D view; the old view's copies went with it)
    assert wc.audit(case.audit_args()) >= case.kinds - ({"V2plain", "T"} if name == "conv1x1" else set())
    case.host()
    assert wc.audit(case.audit_args()) >= case.kinds


def test_lnmlp_replaced_gamma_is_not_a_hit():
    """Writer (g): the entry is keyed by fc1's weight alone; a DIFFERENT gamma Parameter with the same version counter and
    generation must not be served the copies folded from the old one."""
    case = wc.make_cases("cpu", ["lnmlp128"])["lnmlp128"]
    gamma, beta, w1, b1, w2 = case.groups[0].five
    ops._ln_mlp_weights(gamma, beta, w1, b1, w2)
    other = torch.nn.Parameter(gamma.detach() * 2.0 + 1.0)
    assert other._version == gamma._version
    assert "LNMLP" in wc.audit([wc.LNMLP(other, beta, w1, b1, w2)])
    got = ops._ln_mlp_weights(other, beta, w1, b1, w2)
    for g_, want in zip(got, wc.exp_lnmlp(other, beta, w1, b1, w2)):
        assert torch.equal(g_, want.contiguous())


def test_plain_copy_follows_a_device_independent_data_swap():
    """`w.data = other` (what module.to() / module.float() / vector_to_parameters do) keeps the version counter: the storage
    address in the stamp is what tells; and `.data` in-place writes are seen after mark_weights_dirty(), the stated contract."""
    w = torch.nn.Parameter(torch.randn(16, 8))
    a = ops.bf16_weight(w)
    assert torch.equal(a, wc.exp_plain(w))
    v0 = w._version
    w.data = torch.randn(16, 8)
    assert w._version == v0
    assert torch.equal(ops.bf16_weight(w), wc.exp_plain(w)) and torch.equal(ops.bf16_weight_t(w), wc.exp_t(w))
    w.data.mul_(2.0)
    assert w._version == v0
    ops.mark_weights_dirty()
    assert torch.equal(ops.bf16_weight(w), wc.exp_plain(w)) and torch.equal(ops.bf16_weight_t(w), wc.exp_t(w))


def test_audit_fails_on_a_copy_marked_current_with_old_content():
    """The audit can fail: an entry restamped as current without being rewritten."""
    w = torch.nn.Parameter(torch.randn(16, 8))
    ops.bf16_weight_t(w)
    with torch.no_grad():
        w.mul_(3.0)
    ops.bf16_weight(w)
    ent = ops._wcache[("T", id(w))]
    ops._wcache[("T", id(w))] = (ops._stamp(w), ent[1], ent[2])
    with pytest.raises(AssertionError, match="T copy"):
        wc.audit([w])


# ---- the project's own initialisers ---------------------------------------------------------------------------------------------
def _init_modules():
    import torch.nn as nn
    return nn.ModuleList([nn.Linear(24, 40), nn.Embedding(11, 24), nn.LayerNorm(24), nn.Linear(40, 8, bias=False)])


def test_initialisers_draw_the_same_values_as_before():
    """The initialisers write in place under no_grad instead of through `.data`: the values, and the generator draws behind
    them, are those of `torch.empty(shape).normal_(0, 0.02)` etc. from the same seed, in module order."""
    from fiber_amd.modules import dyhead, objectives, roberta
    for fn in (objectives.init_weights, roberta.RobertaModel._init_weights):
        mods = _init_modules()
        torch.manual_seed(5)
        mods.apply(fn)
        torch.manual_seed(5)
        for m in mods:
            if isinstance(m, torch.nn.LayerNorm):
                assert torch.equal(m.weight, torch.ones(24)) and torch.equal(m.bias, torch.zeros(24))
                continue
            assert torch.equal(m.weight.detach(), torch.empty(m.weight.shape).normal_(mean=0.0, std=0.02))
            if getattr(m, "bias", None) is not None:
                assert torch.equal(m.bias.detach(), torch.zeros(m.bias.shape))
        assert all(p.requires_grad and p.grad_fn is None for p in mods.parameters())
    torch.manual_seed(6)
    conv = dyhead.ModulatedDeformConv(16, 27, 3)
    torch.manual_seed(6)
    n = 16 * 9
    assert torch.equal(conv.weight.detach(), torch.empty(27, 16, 3, 3).uniform_(-n ** -0.5, n ** -0.5))
    assert conv.bias is None or torch.equal(conv.bias.detach(), torch.zeros(27))
    head = dyhead.DyConv(16, 16)
    torch.manual_seed(7)
    head.init_weights()
    torch.manual_seed(7)
    convs = [m for m in head.DyConv.modules() if isinstance(m, torch.nn.Conv2d)]
    convs += [m for m in head.AttnConv.modules() if isinstance(m, torch.nn.Conv2d)]
    assert convs
    for m in convs:
        assert torch.equal(m.weight.detach(), torch.empty(m.weight.shape).normal_(0, 0.01))
        assert m.bias is None or torch.equal(m.bias.detach(), torch.zeros(m.bias.shape))


def test_reinitialising_after_a_forward_leaves_no_stale_copy():
    """module.apply(init_weights) AFTER the copies exist (a forward pass made them): the version counters move, the audit passes."""
    from fiber_amd.modules import objectives
    mods = _init_modules()
    lin = mods[0]
    ops.bf16_weight(lin.weight), ops.bf16_weight_t(lin.weight)
    torch.manual_seed(9)
    mods.apply(objectives.init_weights)
    assert not torch.equal(ops._wcache[id(lin.weight)][1], wc.exp_plain(lin.weight))     # the copy IS old ...
    assert wc.audit([lin.weight]) >= {"plain", "T"}                                       # ... and known to be
    assert torch.equal(ops.bf16_weight(lin.weight), wc.exp_plain(lin.weight))
