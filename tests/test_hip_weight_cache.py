"""GPU: every kind of derived weight copy of fiber_amd/ops.py against every way its fp32 master changes, through the ops that
consume the copies (tests/weight_cache_cases.py: expected values, audit, cases, writers).  After each writer the audit must
pass, and the op's next forward output and input gradient must equal, bit for bit, those of the same call on a COLD cache.
FiberAdamW.step() is the one writer that keeps copies current itself (the kernel rewrites the plain copies, two one-launch
refreshes the transposed / head-major ones): pinned by the entries' stamps, their unchanged addresses and the launches made.
Then the cache after hipGraph replays, where no host-side stamping runs, and three mutations the audit must catch."""
import collections

import pytest
import torch

import weight_cache_cases as wc
from tests.hip_util import BF, DEV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from fiber_amd import lib, ops
    lib.load()
    return ops


@pytest.fixture(autouse=True)
def _fresh_cache(ops):
    ops.clear_weight_cache()
    yield
    ops.clear_weight_cache()


@pytest.fixture
def calls(monkeypatch):
    """Names of the lib.call entries made, in order."""
    from fiber_amd import lib
    made, orig = [], lib.call

    def counted(name, *a, **k):
        made.append(name)
        return orig(name, *a, **k)
    monkeypatch.setattr(lib, "call", counted)
    return made


def _use(case):
    """The consuming op, forward and backward (the accessor calls and hand-made gradients for the shape no kernel consumes)."""
    if case.run is not None:
        return case.run()
    case.host()
    wc._give_grads(case)
    return None


def _cold_compare(ops, case, what):
    """The op on the cache as it stands against the op on a cold cache: same output, same input gradient, bit for bit."""
    if case.run is None:
        return
    y1, dx1 = case.run()
    assert wc.audit(case.audit_args()) >= case.kinds
    ops.clear_weight_cache()
    y2, dx2 = case.run()
    assert torch.equal(y1, y2), f"{what}: forward output differs from the cold-cache run ({int((y1 != y2).sum())} elements)"
    assert (dx1 is None and dx2 is None) or torch.equal(dx1, dx2), f"{what}: input gradient differs from the cold-cache run"


def _fast_state(ops, case):
    """(is current, addresses) of every entry FiberAdamW.step() rewrites itself."""
    cur, ptrs = [], []
    for key, w, extra in case.fast + case.slow:
        ent = ops._cache_get(key, w)
        assert ent is not None, (case.name, key)
        cur.append(wc.is_current(ops, key, w, extra))
        ptrs.append([t.data_ptr() for t in (ent[1][:3] if isinstance(ent[1], tuple) else [ent[1]])])
    for s in case.groups:
        if isinstance(s, wc.Pack):
            pk = ops._packs[tuple(id(w) for w in s.ws)]
            cur.append(wc.pack_is_current(ops, s))
            ptrs.append([pk["plain"].data_ptr(), pk["t"].data_ptr(), pk["bias"].data_ptr()])
    return cur, ptrs


@pytest.mark.parametrize("writer", sorted(wc.GPU_WRITERS))
@pytest.mark.parametrize("name", wc.GPU_CASES)
def test_copies_follow_the_writer(ops, name, writer):
    case = wc.make_cases(DEV, [name])[name]
    _use(case)
    assert wc.audit(case.audit_args()) >= case.kinds, "the case did not create the copies it is about"
    wc.GPU_WRITERS[writer](case)
    cur, _ = _fast_state(ops, case)
    assert not any(cur), f"{name} / {writer}: a copy is still called current after a writer that rewrites none"
    _cold_compare(ops, case, f"{name} / {writer} (lazy rebuild inside the op)")
    # once more, this time the audit's accessor calls meet the stale entries, not the op
    _use(case)
    wc.GPU_WRITERS[writer](case)
    seen = wc.audit(case.audit_args())
    assert seen >= case.kinds - ({"V2plain", "T"} if name == "conv1x1" else set())


def _opt(case):
    from fiber_amd.optim import FiberAdamW
    return FiberAdamW(list(case.params), lr=1e-2, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.01)


def _assert_kept_current(ops, case, ptrs0, made, what):
    """After a FiberAdamW.step() in which every member had a gradient: the copies it rewrites are current WITHOUT a lazy rebuild
    (stamps, unchanged addresses, one launch per refresh kernel, nothing else), odd-shaped ones are left to the lazy path."""
    cur, ptrs = _fast_state(ops, case)
    n_slow = len(case.slow)
    n_fast = len(case.fast)
    assert all(cur[:n_fast]) and all(cur[n_fast + n_slow:]), f"{what}: a copy the step rewrites is not marked current"
    assert not any(cur[n_fast:n_fast + n_slow]), f"{what}: a copy the one-launch refresh skips is marked current"
    assert ptrs == ptrs0, f"{what}: a copy moved"
    want = collections.Counter({"fiber_adamw_multi_f32": 1}) + collections.Counter(case.launches)
    assert collections.Counter(made) == want, f"{what}: launches {collections.Counter(made)}"


@pytest.mark.parametrize("situation", ["all_grads", "one_grad_none", "grads_reallocated", "copy_appears_later"])
@pytest.mark.parametrize("name", wc.GPU_CASES)
def test_fiber_adamw_step(ops, calls, name, situation):
    case = wc.make_cases(DEV, [name])[name]
    opt = _opt(case)
    what = f"{name} / FiberAdamW, {situation}"
    _use(case)
    if situation == "copy_appears_later":
        ops.clear_weight_cache()
        opt.step()                                           # no copy exists: the table's copy column is empty
        opt.zero_grad(set_to_none=False)
        _use(case)                                           # the copies appear (built from the updated masters)
    elif situation == "grads_reallocated":
        opt.step()
        opt.zero_grad(set_to_none=True)
        _use(case)
    elif situation == "one_grad_none":
        case.params[0].grad = None
    assert wc.audit(case.audit_args()) >= case.kinds
    _, ptrs0 = _fast_state(ops, case)
    before = [p.detach().clone() for p in case.params]
    del calls[:]
    opt.step()
    made = list(calls)
    moved = [not torch.equal(a, p.detach()) for a, p in zip(before, case.params)]
    if situation == "one_grad_none":
        assert not moved[0] and all(moved[1:]) if len(moved) > 1 else not moved[0]
        assert made.count("fiber_adamw_multi_f32") == (1 if len(moved) > 1 else 0)
    else:
        assert all(moved)
        _assert_kept_current(ops, case, ptrs0, made, what)
    assert wc.audit(case.audit_args()) >= case.kinds
    _cold_compare(ops, case, what)


def test_replaced_bias_and_gamma_are_not_hits(ops):
    """Writer (g): a DIFFERENT Parameter object with the same version counter in place of the qkv bias / of LayerNorm's gamma."""
    cases = wc.make_cases(DEV, ["qkv64", "lnmlp128"])
    q = cases["qkv64"]
    q.run()
    s = q.groups[0]
    other = torch.nn.Parameter(s.b.detach() * 2.0 + 1.0)
    assert other._version == s.b._version
    x = torch.randn(64, 64, device=DEV).to(BF)
    assert "HM" in wc.audit([wc.HM(s.w, other, s.heads)])
    y1 = ops.linear_qkv_head_major(x, s.w, other, s.heads)
    ops.clear_weight_cache()
    assert torch.equal(y1, ops.linear_qkv_head_major(x, s.w, other, s.heads))
    ln = cases["lnmlp128"]
    ln.run()
    gamma, beta, w1, b1, w2 = ln.groups[0].five
    b2 = ln.params[5]
    other = torch.nn.Parameter(gamma.detach() * 2.0 + 1.0)
    assert other._version == gamma._version
    x = torch.randn(100, 128, device=DEV).to(BF)
    y1 = ops.ln_mlp(x, other, beta, 1e-5, w1, b1, w2, b2)
    assert "LNMLP" in wc.audit([wc.LNMLP(other, beta, w1, b1, w2)])
    ops.clear_weight_cache()
    assert torch.equal(y1, ops.ln_mlp(x, other, beta, 1e-5, w1, b1, w2, b2))


def test_copies_follow_a_move_between_devices(ops):
    """A copy made on the host is not handed to a parameter that has moved to the GPU since (`module.to()` keeps id and version)."""
    w = torch.nn.Parameter(torch.randn(16, 8))
    ops.bf16_weight(w), ops.bf16_weight_t(w)
    w.data = w.data.to(DEV)
    assert ops.bf16_weight(w).device == w.device and ops.bf16_weight_t(w).device == w.device
    assert wc.audit([w]) >= {"plain", "T"}


# ---- hipGraph replay: no host-side stamping runs --------------------------------------------------------------------------------
def test_cache_after_graph_replay(ops):
    """The TINY model and batch of tests/test_hip_graph.py, captured after one warm-up step.  After each of two replays the copies
    FiberAdamW's kernels rewrite (plain, transposed, head-major, packs) hold the CURRENT masters; the copies the forward rebuilds
    lazily hold either the current masters or those from before the replay -- which of the two is recorded per kind and must
    not change from one replay to the next.  After close() one eager forward must leave a cache that passes the audit."""
    from fiber_amd import parallel
    from fiber_amd.config import make_config
    from fiber_amd.graph import GraphedTrainStep
    from fiber_amd.modules import FIBERTransformerSS, fiber_utils
    from oracle import cases, detgen
    ops.disable_graph_rng()
    torch.manual_seed(0)
    cfg = dict(cases.TINY, text_dropout=0.1, drop_path_rate=0.1)
    model = FIBERTransformerSS(make_config(**cfg, learning_rate=1e-3, lr_mult_head=5, lr_mult_cross_modal=5, warmup_steps=3,
                                           max_steps=20, weight_decay=0.01, end_lr=0, decay_power=1))
    detgen.fill_(model)
    for n, p in model.named_parameters():
        if "alpha_" in n:
            p.data.fill_(0.5)
    parallel.freeze_unused(model, model.unused_parameter_names())
    model.to("cuda").train()
    fiber_utils.set_task(model)
    ops.manual_seed(3)
    (opt,), (sched,) = model.configure_optimizers()
    b = detgen.synth_batch(4, 96, 12, 1000, seed=11, min_len=6)
    bd = {k: (v.cuda() if isinstance(v, torch.Tensor) else [t.cuda() for t in v] if isinstance(v, list) and isinstance(v[0], torch.Tensor) else v)
          for k, v in b.items()}
    bd["itm_labels_override"] = bd["itm_labels"].clone()
    g = GraphedTrainStep(model, opt, sched, bd, warmup=1)
    bias_of = {id(m.weight): m.bias for m in model.modules() if isinstance(m, torch.nn.Linear)}
    trained = [p for p in model.parameters() if p.requires_grad]
    which = []
    try:
        for replay in range(2):
            pre = {id(p): p.detach().clone() for p in model.parameters()}
            for key, ent in list(ops._wcache.items()):                 # the 2-D views of 1x1 convs own copies of their own
                if isinstance(key, tuple) and key[0] == "V2" and ent[2]() is not None:
                    pre[id(ent[1])] = pre[id(ent[2]())].view(ent[1].shape)
            g()
            torch.cuda.synchronize()
            assert any(not torch.equal(pre[id(p)], p.detach()) for p in trained), "the replay did not train"
            rec = {}
            for key, ent in list(ops._wcache.items()):
                pairs_now = wc.entry_pairs(ops, key, ent)
                if pairs_now is None:
                    continue
                kind = key[0] if isinstance(key, tuple) else ("plain" if isinstance(ent[2](), torch.nn.Parameter) else "V2plain")
                name = f"replay {replay}: {kind} copy of {tuple(ent[2]().shape)}"
                if kind in wc.PLAIN_KINDS:
                    assert wc.pairs_equal(pairs_now), name + " does not hold the current master"
                    rec.setdefault(kind, set()).add("current")
                else:
                    now, old = wc.pairs_equal(pairs_now), wc.pairs_equal(wc.entry_pairs(ops, key, ent, m=lambda t: pre[id(t)]))
                    assert now or old, name + " holds neither the current master nor the one from before the replay"
                    if not (now and old):                              # (a frozen parameter: both at once, says nothing)
                        rec.setdefault(kind, set()).add("current" if now else "before the replay")
            for pk in list(ops._packs.values()):
                ws = [r() for r in pk["refs"]]
                if any(w is None for w in ws):
                    continue
                plain, t, bias = wc.exp_pack(ws, [bias_of[id(w)] for w in ws])
                assert torch.equal(pk["plain"], plain) and torch.equal(pk["t"], t.contiguous()), f"replay {replay}: pack is not current"
                assert bias is None or torch.equal(pk["bias"], bias), f"replay {replay}: packed bias"
                rec.setdefault("pack", set()).add("current")
            which.append(rec)
    finally:
        g.close()
    print("weight cache after replay, per kind:", {k: sorted(v) for k, v in which[0].items()})
    assert which[0] == which[1], which
    assert all(len(v) == 1 for v in which[0].values()), which[0]
    # the TINY model has all of these: window blocks (HM), RoBERTa q / k / v (packs), a C = 128 Swin stage (LNMLP), the patch embedding
    assert {"plain", "T", "HM", "pack", "LNMLP", "pe"} <= set(which[0]), which[0]
    # the lazily rebuilt kinds are rebuilt by the captured FORWARD, which precedes that replay's update of the masters
    assert all(v == {"before the replay"} for k, v in which[0].items() if k in wc.LAZY_KINDS), which[0]
    model.global_step = g.step_index
    ops.set_rng_step(g.step_index)
    with torch.no_grad():
        model.training_step(bd, g.step_index)
    packs = [wc.Pack(ws, [bias_of[id(w)] for w in ws]) for ws in ([r() for r in pk["refs"]] for pk in ops._packs.values())]
    seen = wc.audit(packs)
    assert seen >= set(which[0]), (seen, which[0])


# ---- the audit must be able to fail ---------------------------------------------------------------------------------------------
def test_mutation_transposed_copies_marked_current_without_launch(ops, monkeypatch):
    def marks_only():
        for key, (stamp, wt, ref) in list(ops._wcache.items()):
            if isinstance(key, tuple) and key[0] == "T" and ref() is not None:
                ops._wcache[key] = (ops._stamp(ref()), wt, ref)
    monkeypatch.setattr(ops, "refresh_transposed_copies", marks_only)
    case = wc.make_cases(DEV, ["linear64"])["linear64"]
    case.run()
    _opt(case).step()
    with pytest.raises(AssertionError, match="T copy of"):
        wc.audit(case.audit_args())


def test_mutation_restamp_does_not_bump_the_generation(ops, monkeypatch):
    orig = ops.restamp_bf16_copies
    monkeypatch.setattr(ops, "restamp_bf16_copies", lambda params, bump=True: orig(params, bump=False))
    case = wc.make_cases(DEV, ["lnmlp128"])["lnmlp128"]
    case.run()
    _opt(case).step()
    with pytest.raises(AssertionError, match="LNMLP copy of"):
        wc.audit(case.audit_args())


def test_mutation_pack_transpose_not_rewritten_after_member_refresh(ops, monkeypatch):
    orig = ops._pack_get

    def keeps_old_transpose(weights, biases):
        pk0 = ops._packs.get(tuple(id(w) for w in weights))
        old = pk0["t"].clone() if pk0 is not None else None
        pk = orig(weights, biases)
        if old is not None and pk is pk0:
            pk["t"].copy_(old)                               # as if the `pk["t"]` rewrite had been skipped; t_stamp says current
        return pk
    monkeypatch.setattr(ops, "_pack_get", keeps_old_transpose)
    case = wc.make_cases(DEV, ["pack3"])["pack3"]
    case.run()
    wc.w_copy(case)
    with pytest.raises(AssertionError, match="pack of 3 .*transpose"):
        wc.audit(case.audit_args())
