"""Host-only checks of the grounding solver (fiber_amd/solver.py, tests/solver_cases.py): the fp64 restatement of the solver kernels against
torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(foreach=False) run in fp64 over three consecutive steps; four mutations of the rule
that a whole-tensor rel-L2 of 1e-2 accepts and the per-element bounds (K at the operation counts) reject; make_optimizer's groups on the
test detector; the schedules against their closed forms; the host ModelEma; the settings that are refused."""
import math
import types

import numpy as np
import pytest
import torch

from tests import solver_cases as sc

T64 = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))      # noqa: E731
ns = types.SimpleNamespace


def rel_l2(a, b):
    """in fp64: the squares of the 1e15 gradients' moments leave fp32"""
    return float((a - b).norm() / (b.norm() + 1e-300))


def solver_cfg(**over):
    s = dict(OPTIMIZER="ADAMW", BASE_LR=1e-4, LANG_LR=1e-5, BACKBONE_BODY_LR_FACTOR=0.5, BIAS_LR_FACTOR=2, WEIGHT_DECAY=0.05, WEIGHT_DECAY_BIAS=0.0,
             WEIGHT_DECAY_NORM_FACTOR=0.25, MODEL_EMA=0.999, MAX_ITER=100, STEPS=(6, 8), GAMMA=0.1, WARMUP_ITERS=4, WARMUP_FACTOR=0.001,
             WARMUP_METHOD="linear", USE_COSINE=False, USE_AUTOSTEP=False, MULTI_MAX_EPOCH=(), MIN_LR=0.0, WEIGHT_DECAY_SCHEDULE=False,
             WEIGHT_DECAY_SCHEDULE_RATIO=0.667)
    clip = dict(ENABLED=True, CLIP_VALUE=1.0, CLIP_TYPE="full_model", NORM_TYPE=2.0)
    for k, v in over.items():
        (clip if k in clip else s)[k] = v
    return ns(SOLVER=ns(CLIP_GRADIENTS=ns(**clip), **s))


# ---- the restatement against torch in fp64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in sc.CASES])
def test_restatement_matches_torch_adamw_in_fp64(name):
    """betas whose complements are exact in fp32 (the kernel forms 1 - b in fp32); lr, wd, eps, max_norm at their fp32 values.  Each of
    three consecutive steps agrees within 1e-12 of the magnitude of the terms summed (the bound term of each quantity)."""
    case = dict(sc.BY_NAME[name], b1=0.875, b2=0.96875)
    state = [{k: a.astype(np.float64) for k, a in st.items()} for st in sc.make_state(case)]
    steps = sc.prior_steps(case)
    if case.get("inf"):
        # the composition the kernels replace does not step on non-finite gradients (GradScaler.step): nothing moves but the EMA
        out = sc.reference_step(case, state)
        assert out["skip"] == 1 and out["c"] == 0.0 and np.array_equal(out["steps"], steps)
        for i, (st, d) in enumerate(zip(state, out["tensors"])):
            assert all(np.array_equal(d[k], st[k]) for k in ("p", "m", "v"))
            if sc.has_ema(case, i):
                assert np.array_equal(d["ema"], sc.ema_reference(case, st["ema"], st["p"])[0])
        return
    rows = sc.hyper_rows(case).astype(np.float64)
    params = [torch.nn.Parameter(T64(st["p"])) for st in state]
    opt = torch.optim.AdamW([{"params": [p], "lr": float(r[0]), "weight_decay": float(r[1])} for p, r in zip(params, rows)], lr=1e-3,
                            betas=(case["b1"], case["b2"]), eps=sc.f32(case["eps"]), foreach=False)
    for p, st, t in zip(params, state, steps):
        opt.state[p].update(step=torch.tensor(float(t)), exp_avg=T64(st["m"]), exp_avg_sq=T64(st["v"]))
    for k in range(3):
        for p, st in zip(params, state):
            p.grad = T64(st["g"])
        if case["max_norm"] is not None:
            torch.nn.utils.clip_grad_norm_(params, sc.f32(case["max_norm"]), foreach=False)
        opt.step()
        out = sc.reference_step(case, state, steps_before=steps + k)
        assert (out["c"] == 1.0) == (case["max_norm"] is None or case["max_norm"] > 1e18)
        for i, (p, st, d) in enumerate(zip(params, state, out["tensors"])):
            m1, v1, tm, tv = sc.moments_reference(case, st, out["c"])
            _, tp = sc.param_reference(case, st["p"], m1, v1, out["coef"][i])
            os_ = opt.state[p]
            assert int(os_["step"]) == out["steps"][i]
            for what, got, ref, term in (("m", os_["exp_avg"], d["m"], tm), ("v", os_["exp_avg_sq"], d["v"], tv), ("p", p.detach(), d["p"], tp)):
                err = (got - T64(ref)).abs()
                assert bool((err <= 1e-12 * T64(term) + 1e-300).all()), (name, k, i, what, float((err / T64(term).clamp_min(1e-300)).max()))
        state = [dict(st, p=d["p"], m=d["m"], v=d["v"], ema=d.get("ema", st["ema"])) for st, d in zip(state, out["tensors"])]


def test_the_cases_hold_what_they_promise():
    assert sc.K == {"M": 8.0, "V": 10.0, "P": 14.0, "EMA": 6.0}
    n_chunks = len(sc.chunk_table())
    assert n_chunks > 256 + 12 and len(sc.TENSORS) > 256 and sc.TENSORS[12][0] == 300 * 4096 + 5
    assert sorted(set(sc.chunk_table())) == sorted(sc.chunk_table()) and sum(-(-t[0] // sc.CHUNK) for t in sc.TENSORS) == n_chunks
    assert {t[0] for t in sc.TENSORS[13:]} == set(range(1, 8))
    norms = {c["name"]: sc.scalars_reference(c, sc.make_state(c)) for c in sc.CASES}
    assert norms["mixed_above_some"][1] == 1.0 and norms["step1_off_ema"][1] == 1.0
    assert 0.01 < norms["mixed_below_ema"][1] < 0.5 and norms["inf_some"][1:] == (0.0, 1)
    assert math.isfinite(norms["mixed_below_ema"][0]) and np.isfinite(np.float32(norms["mixed_below_ema"][0] ** 2))
    some = [sc.has_ema(sc.BY_NAME["mixed_above_some"], i) for i in range(len(sc.TENSORS))]
    assert any(some) and not all(some)
    assert len(set(sc.prior_steps(sc.BY_NAME["mixed_above_some"]).tolist())) == 3 and len({tuple(r) for r in sc.hyper_rows(sc.BY_NAME["mixed_above_some"])}) == 12


# ---- mutations ----------------------------------------------------------------------------------------------------------------------------------
def _mutation_case(mutate):
    case = sc.BY_NAME["mixed_below_ema"]
    if mutate == "c_m_only":                     # c = 0.999: a clip that rel-L2 1e-2 cannot see on v'
        norm = sc.scalars_reference(case, sc.make_state(case))[0]
        case = dict(case, max_norm=0.999 * norm)
    return case


@pytest.mark.parametrize("mutate", ["decay_after", "eps_before", "c_m_only", "ema_from_p"])
def test_mutation_is_rejected_by_the_bounds_and_accepted_by_rel_l2(mutate):
    case = _mutation_case(mutate)
    state = sc.make_state(case)
    ref, mut = sc.reference_step(case, state), sc.reference_step(case, state, mutate=mutate)
    sc.verify_step(case, state, ref)                             # the restatement itself passes its own bounds
    changed = 0
    for i, (a, b) in enumerate(zip(mut["tensors"], ref["tensors"])):
        for k in b:
            e = rel_l2(T64(a[k]), T64(b[k]))
            assert e <= 1e-2, f"{mutate}: tensor {i} {k} rel-L2 {e:.3e}: not a mutation the whole-tensor tolerance accepts"
            changed += not np.array_equal(a[k], b[k])
    assert changed, f"{mutate}: the mutation changed nothing"
    with pytest.raises(AssertionError, match={"decay_after": " P", "eps_before": " P", "c_m_only": " V", "ema_from_p": " EMA"}[mutate]):
        sc.verify_step(case, state, mut)


# ---- make_optimizer -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_detector():
    import fpn_cases as fc
    from fiber_amd.modules import GeneralizedVLRCNN
    torch.manual_seed(0)
    return GeneralizedVLRCNN(fc.model_cfg())


PINNED = {
    "fusion_backbone.backbone.body.patch_embed.proj.weight": (5e-5, 0.05),                                            # body
    "fusion_backbone.backbone.body.layers.0.blocks.0.attn.relative_position_bias_table": (1e-4, 0.0),                 # body + "bias" (not a bias)
    "fusion_backbone.backbone.body.patch_embed.norm.weight": (5e-5, 0.0125),                                          # body + norm
    "fusion_backbone.backbone.body.patch_embed.norm.bias": (1e-4, 0.0),                                               # body + bias + norm
    "fusion_backbone.backbone.fpn.fpn_inner2.weight": (1e-4, 0.05),                                                   # plain
    "fusion_backbone.backbone.fpn.fpn_inner2.bias": (2e-4, 0.0),                                                      # bias
    "fusion_backbone.language_backbone.body.model.embeddings.word_embeddings.weight": (1e-5, 0.05),                   # lang
    "fusion_backbone.language_backbone.body.model.embeddings.LayerNorm.weight": (1e-5, 0.0125),                       # lang + norm
    "fusion_backbone.language_backbone.body.model.embeddings.LayerNorm.bias": (2e-5, 0.0),                            # lang + bias + norm
    "fusion_backbone.language_backbone.body.model.encoder.layer.0.attention.self.query.bias": (2e-5, 0.0),            # lang + bias
}


def test_make_optimizer_groups(host_detector):
    from fiber_amd.solver import ClippedAdamW, make_optimizer
    cfg = solver_cfg()
    opt = make_optimizer(cfg, host_detector)
    named = dict(host_detector.named_parameters())
    assert len(named) == 460 and sum(not p.requires_grad for p in named.values()) == 2
    assert isinstance(opt, ClippedAdamW) and isinstance(opt, torch.optim.AdamW) and opt.max_grad_norm == 1.0
    assert len(opt.param_groups) == 458 and all(len(g["params"]) == 1 for g in opt.param_groups)
    assert all(g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8 for g in opt.param_groups)
    by_id = {id(g["params"][0]): (g["lr"], g["weight_decay"]) for g in opt.param_groups}
    trainable = [n for n, p in named.items() if p.requires_grad]
    assert [id(g["params"][0]) for g in opt.param_groups] == [id(named[n]) for n in trainable]       # model order
    for key, (lr, wd) in PINNED.items():
        got = by_id[id(named[key])]
        assert got == pytest.approx((lr, wd), rel=1e-12, abs=0.0), (key, got)
    assert not any(id(p) in by_id for p in host_detector.rpn.head.cls_logits.parameters())
    for off in (dict(ENABLED=False), dict(CLIP_VALUE=0.0)):
        assert make_optimizer(solver_cfg(**off), host_detector).max_grad_norm is None


def test_clipped_adamw_is_clip_then_adamw():
    from fiber_amd.solver import ClippedAdamW
    g_ = torch.Generator().manual_seed(3)
    ps = [torch.randn(7, generator=g_).double() for _ in range(3)]
    gs = [torch.randn(7, generator=g_).double() * 3 for _ in range(3)]
    a = [torch.nn.Parameter(p.clone()) for p in ps]
    b = [torch.nn.Parameter(p.clone()) for p in ps]
    oa = ClippedAdamW([{"params": [p], "lr": 1e-2 * (i + 1), "weight_decay": 0.1 * i} for i, p in enumerate(a)], 1e-3, max_grad_norm=0.5)
    ob = torch.optim.AdamW([{"params": [p], "lr": 1e-2 * (i + 1), "weight_decay": 0.1 * i} for i, p in enumerate(b)], 1e-3)
    for _ in range(2):
        for p, q, g in zip(a, b, gs):
            p.grad, q.grad = g.clone(), g.clone()
        oa.step()
        torch.nn.utils.clip_grad_norm_(b, 0.5)
        ob.step()
    assert all(torch.equal(p, q) for p, q in zip(a, b))


# ---- schedules ------------------------------------------------------------------------------------------------------------------------------------
def _lrs(sched, opt, n):
    out = []
    for _ in range(n):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return out


def _sgd(lr=1.0):
    return torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)


def test_warmup_multistep_schedule():
    from fiber_amd.solver import WarmupMultiStepLR, make_lr_scheduler
    opt = _sgd()
    sched = make_lr_scheduler(solver_cfg(), opt)
    assert isinstance(sched, WarmupMultiStepLR) and sched.milestones == [6, 8] and sched.gamma == 0.1
    assert _lrs(sched, opt, 10) == pytest.approx([0.001, 0.25075, 0.5005, 0.75025, 1, 1, 0.1, 0.1, 0.01, 0.01], rel=1e-12)
    frac = make_lr_scheduler(solver_cfg(STEPS=(0.67, 0.89), MAX_ITER=100), _sgd())
    assert frac.milestones == [67, 89]
    const = make_lr_scheduler(solver_cfg(WARMUP_METHOD="constant"), o2 := _sgd())
    assert _lrs(const, o2, 5) == pytest.approx([0.001] * 4 + [1.0], rel=1e-12)
    # state_dict round trip: a fresh scheduler continues where the first stood
    opt_a, opt_b = _sgd(), _sgd()
    a = make_lr_scheduler(solver_cfg(), opt_a)
    _lrs(a, opt_a, 5)
    b = make_lr_scheduler(solver_cfg(), opt_b)
    b.load_state_dict(a.state_dict())
    assert b.last_epoch == a.last_epoch == 5 and b.milestones == a.milestones
    opt_b.param_groups[0]["lr"] = opt_a.param_groups[0]["lr"]
    assert _lrs(a, opt_a, 5) == _lrs(b, opt_b, 5)


def test_warmup_cosine_schedule():
    from fiber_amd.solver import WarmupCosineAnnealingLR, make_lr_scheduler
    opt = _sgd(2.0)
    sched = make_lr_scheduler(solver_cfg(USE_COSINE=True, MAX_ITER=20, MIN_LR=0.1), opt)
    assert isinstance(sched, WarmupCosineAnnealingLR)
    lrs = _lrs(sched, opt, 25)
    for it in (0, 3, 4, 14, 24):
        want = 2.0 * (0.001 * (1 - it / 4) + it / 4) if it < 4 else 0.1 + (2.0 - 0.1) * (1 + math.cos(math.pi * (it - 4) / 20)) / 2
        assert lrs[it] == pytest.approx(want, rel=1e-12), it


# ---- the host EMA ---------------------------------------------------------------------------------------------------------------------------------
class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(5, 3)
        self.norm = torch.nn.LayerNorm(3)
        self.register_buffer("position_ids", torch.arange(7))
        self.register_buffer("scale", torch.ones(3))


def test_host_model_ema():
    from fiber_amd.solver import ModelEma
    torch.manual_seed(1)
    model = _Tiny().train()
    d = 0.9
    ema = ModelEma(model, d)
    assert ema.decay == d and not ema.ema.training and not any(p.requires_grad for p in ema.ema.parameters())
    assert all(ema.ema_of(p) is e for p, e in zip(model.parameters(), ema.ema.parameters())) and ema.ema_of(torch.zeros(1)) is None
    snaps = [{k: v.clone() for k, v in model.state_dict().items()}]
    for k in range(3):
        with torch.no_grad():
            for p in model.parameters():
                p.add_(torch.randn_like(p))
            model.scale.mul_(1.5)
            model.position_ids.add_(100003)                     # an integer an fp32 average would not carry
        snaps.append({k_: v.clone() for k_, v in model.state_dict().items()})
        ema.update(model)
    sd = ema.state_dict()
    assert set(sd) == set(snaps[0])
    for k, e in sd.items():
        if e.is_floating_point():
            p0, p1, p2, p3 = (s[k].double() for s in snaps)
            want = d ** 3 * p0 + (1 - d) * (d ** 2 * p1 + d * p2 + p3)
            assert float((e.double() - want).abs().max()) <= 1e-6 * float(want.abs().max()), k
        else:
            assert torch.equal(e, snaps[3][k]) and e.dtype == snaps[3][k].dtype, k
    other = ModelEma(_Tiny(), d)
    other.load_checkpoint({"model_ema": {"module." + k: v for k, v in sd.items()}})
    assert all(torch.equal(v, sd[k]) for k, v in other.state_dict().items())
    other.load_checkpoint({"model": {}})                         # no "model_ema" entry: nothing to load
    wrapped = ns(module=model)                                   # a DDP-style wrapper
    ema.update(wrapped)


def test_host_grounding_solver_step():
    """the iteration on a host model: NaN total zeroed, warm-up followed, the weight-decay schedule fires once, the EMA follows"""
    from fiber_amd.solver import ClippedAdamW, GroundingSolver
    torch.manual_seed(2)
    model = _Tiny()
    cfg = solver_cfg(WEIGHT_DECAY_SCHEDULE=True, WEIGHT_DECAY_SCHEDULE_RATIO=0.5, MODEL_EMA=0.5)
    solver = GroundingSolver(cfg, model)
    assert isinstance(solver.optimizer, ClippedAdamW) and solver.model_ema is not None
    wd0 = [g["weight_decay"] for g in solver.optimizer.param_groups]
    x = torch.randn(4, 5)
    for it in range(4):
        before = model.fc.weight.detach().clone()
        y = model.norm(model.fc(x))
        losses = {"a": y.square().mean(), "b": y.sum() * 0.1 + (float("nan") if it == 1 else 0.0)}
        out = solver.step(losses)
        assert set(out) == {"a", "b"} and not any(v.requires_grad for v in out.values())
        assert torch.isfinite(model.fc.weight).all()
        assert not torch.equal(model.fc.weight, before)           # (under the zeroed total of iteration 1: by the decay and the moments)
    assert solver.scheduler.last_epoch == 4
    # milestone 6 x ratio 0.5 = 3: fired when last_epoch reached 3, then waits for 8 x 0.5 = 4: fired again at 4
    assert [g["weight_decay"] for g in solver.optimizer.param_groups] == pytest.approx([w * 0.01 for w in wd0])
    assert solver.milestone_target == 2
    sd = solver.state_dict()
    assert set(sd) == {"optimizer", "scheduler", "milestone_target", "model_ema"}
    solver.load_state_dict(sd)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over, word", [(dict(OPTIMIZER="SGD"), "OPTIMIZER"), (dict(NORM_TYPE=1.0), "NORM_TYPE"), (dict(CLIP_TYPE="value"), "CLIP_TYPE")])
def test_unsupported_optimizer_settings_raise(over, word):
    from fiber_amd.solver import make_optimizer
    with pytest.raises(NotImplementedError, match=word):
        make_optimizer(solver_cfg(**over), _Tiny())


@pytest.mark.parametrize("over, word", [(dict(MULTI_MAX_EPOCH=(2, 2)), "MULTI_MAX_EPOCH"), (dict(USE_AUTOSTEP=True), "USE_AUTOSTEP")])
def test_unsupported_schedules_raise(over, word):
    from fiber_amd.solver import make_lr_scheduler
    with pytest.raises(NotImplementedError, match=word):
        make_lr_scheduler(solver_cfg(**over), _sgd())
