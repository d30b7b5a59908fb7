"""GPU tests of the grounding solver: the three entry points of csrc/solver.hip through the C ABI with the hand-built tables of
tests/solver_cases.py (every element of exp_avg, exp_avg_sq, p and the EMA against fp64 within the operation-count bounds, the bf16 copy to the
bit, guards, the scalars and coefficient rows, the device step counts), run-to-run determinism, the skipped non-finite step and the step after
it, fiber_ema_multi_f32 alone; optim.FiberTorchAdamW against torch.optim.AdamW's state dict in both directions and with a parameter that
joins late; solver.GroundingSolver end to end on the test detector, without a host synchronisation, the EMA against its closed form and the
EMA model's cached bf16 copies refreshed.  FIBER_SOLVER_CALIBRATE=<file> records the largest K each bound needed."""
import copy
import json
import os
import types

import numpy as np
import pytest
import torch

import fpn_cases as fc
from tests import solver_cases as sc
from tests.hip_util import DEV, assert_elementwise

pytestmark = pytest.mark.gpu

_CAL = os.environ.get("FIBER_SOLVER_CALIBRATE")
_needed = {}
ns = types.SimpleNamespace


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from fiber_amd import lib
    lib.load()
    return lib


def _record(kind, need):
    if need > _needed.get(kind, 0.0):
        _needed[kind] = need
        if _CAL:
            with open(_CAL, "w") as f:
                json.dump(_needed, f, indent=1)


def T64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).reshape(-1, 1)


def _check_copies(case, out, skipped=False):
    for i, (t, d) in enumerate(zip(sc.TENSORS, out["tensors"])):
        if "w" in d:
            want = np.full(t[0], sc.bf16_bits(np.float32([sc.SENTINEL]))[0], np.uint16) if skipped else sc.bf16_bits(d["p"])
            assert np.array_equal(d["w"].view(np.uint16), want), f"{case['name']} tensor {i}: the bf16 copy is not bf16 of the stored p"


# ---- the kernels through the C ABI -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in sc.CASES])
def test_solver_step(lib, name):
    case = sc.BY_NAME[name]
    state = sc.make_state(case)
    ctx = sc.build(case, state)
    out = sc.launch(lib, case, ctx)
    print(f"{name}: norm {out['norm']:.9g} c {out['c']:.9g} skip {out['skip']}")
    sc.verify_step(case, state, out, record=_record)
    print(f"{name}: largest K needed so far {_needed}")
    skipped = bool(case.get("inf"))
    assert out["skipped"] == (1 if skipped else 0)
    _check_copies(case, out, skipped)
    for i, (st, d) in enumerate(zip(state, out["tensors"])):
        assert np.array_equal(d["g"].view(np.int32), st["g"].view(np.int32)), f"{name} tensor {i}: the gradient was written"
    assert sc.guards_untouched(ctx) == []
    if not skipped:                                              # the partials: each chunk's own sum, to fp64 rounding
        for k, (t, c) in enumerate(sc.chunk_table()):
            g = state[t]["g"][c * sc.CHUNK:(c + 1) * sc.CHUNK].astype(np.float64)
            want = float(np.sum(g * g))
            assert abs(out["partial"][k] - want) <= 1e-12 * want, (name, t, c)


def test_max_norm_above_the_norm_is_clipping_off_to_the_bit(lib):
    case = sc.BY_NAME["mixed_above_some"]
    state = sc.make_state(case)
    a = sc.launch(lib, case, sc.build(case, state))
    b = sc.launch(lib, dict(case, max_norm=None), sc.build(case, state))
    assert a["c"] == 1.0 and b["c"] == 1.0 and a["norm"] == b["norm"]
    for i, (x, y) in enumerate(zip(a["tensors"], b["tensors"])):
        assert set(x) == set(y)
        for k in x:
            assert np.array_equal(x[k].view(np.int16 if k == "w" else np.int32), y[k].view(np.int16 if k == "w" else np.int32)), f"tensor {i} {k}"


def test_two_runs_are_bitwise_identical(lib):
    case = sc.BY_NAME["mixed_below_ema"]
    state = sc.make_state(case)
    a = sc.launch(lib, case, sc.build(case, state))
    b = sc.launch(lib, case, sc.build(case, state))
    assert a["norm"] == b["norm"] and a["c"] == b["c"] and 0.0 < a["c"] < 1.0
    assert np.array_equal(a["partial"].view(np.int64), b["partial"].view(np.int64)) and np.array_equal(a["coef"].view(np.int32), b["coef"].view(np.int32))
    for i, (x, y) in enumerate(zip(a["tensors"], b["tensors"])):
        for k in x:
            assert np.array_equal(x[k].view(np.int16 if k == "w" else np.int32), y[k].view(np.int16 if k == "w" else np.int32)), f"tensor {i} {k}"


def test_skipped_step_then_a_finite_one(lib):
    """the inf gradient: skip = 1, p / m / v / copy / counts as they were, skipped_steps = 1, the EMA moved with the old p (all in
    verify_step); the same tables again with the element made finite: the counts advance by exactly one and the step is the ordinary one"""
    case = sc.BY_NAME["inf_some"]
    state = sc.make_state(case)
    ctx = sc.build(case, state)
    first = sc.launch(lib, case, ctx)
    sc.verify_step(case, state, first)
    assert first["skip"] == 1 and first["skipped"] == 1 and np.array_equal(first["steps"], sc.prior_steps(case))
    _check_copies(case, first, skipped=True)
    t, e = sc.INF_AT
    ctx["bufs"][t]["g"][e] = 0.25
    state2 = [dict(st, ema=d.get("ema", st["ema"])) for st, d in zip(state, first["tensors"])]
    g = state[t]["g"].copy()
    g[e] = 0.25
    state2[t] = dict(state2[t], g=g)
    case2 = dict(case, inf=False, name="after_inf")
    second = sc.launch(lib, case2, ctx)
    sc.verify_step(case2, state2, second, steps_before=sc.prior_steps(case), record=_record)
    assert second["skip"] == 0 and second["skipped"] == 1 and np.array_equal(second["steps"], sc.prior_steps(case) + 1)
    _check_copies(case2, second)
    assert sc.guards_untouched(ctx) == []


def test_ema_multi_alone(lib):
    """fiber_ema_multi_f32 over {src, ema} pairs at every alignment, two launches: each within the EMA bound of the stored value before"""
    shapes = [(1, 0, 0), (5, 4, 0), (7, 0, 8), (4096, 0, 0), (4099, 0, 0), (2 * 4096 + 6, 12, 12)]
    g_ = torch.Generator().manual_seed(9)
    case = dict(d=0.999)
    bufs = []
    for n, soff, eoff in shapes:
        s, e = torch.randn(n, generator=g_), torch.randn(n, generator=g_)
        sb, sv = sc._view(n, soff, torch.float32, s.to(DEV), DEV)
        eb, ev = sc._view(n, eoff, torch.float32, e.to(DEV), DEV)
        bufs.append((sb, sv, eb, ev, s.numpy(), e.numpy()))
    table = torch.tensor([[b[1].data_ptr(), b[3].data_ptr()] for b in bufs], dtype=torch.int64).to(DEV)
    numel = torch.tensor([s[0] for s in shapes], dtype=torch.int64).to(DEV)
    chunks = [(i, c) for i, s in reversed(list(enumerate(shapes))) for c in range(-(-s[0] // sc.CHUNK))]
    chunks_dev = torch.tensor(chunks, dtype=torch.int32).to(DEV)
    for _ in range(2):
        lib.call("fiber_ema_multi_f32", lib.ptr(table), lib.ptr(numel), lib.ptr(chunks_dev), len(chunks), sc.f32(0.999))
        torch.cuda.synchronize()
        for i, (sb, sv, eb, ev, s, e) in enumerate(bufs):
            ref, term = sc.ema_reference(case, e, s)
            assert_elementwise(f"ema pair {i}", T64(ev.cpu().numpy()), T64(ref), T64(sc.K["EMA"] * sc.F32 * term + sc.TINY32))
            assert np.array_equal(sv.cpu().numpy(), s), f"pair {i}: the source was written"
            for buf, view in ((sb, sv), (eb, ev)):
                lead = (view.data_ptr() - buf.data_ptr()) // 4
                assert bool((torch.cat([buf[:lead], buf[lead + view.numel():]]) == sc.SENTINEL).all()), f"pair {i}: written outside the tensor"
            bufs[i] = (sb, sv, eb, ev, s, ev.cpu().numpy())


def test_entry_points_refuse_and_accept_nothing(lib):
    L, P = lib.load(), lib.ptr
    s = torch.cuda.current_stream().cuda_stream
    block = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert L.fiber_grad_sqnorm_multi_f32(None, None, None, 0, None, s) == 0
    assert L.fiber_adamw_torch_multi_f32(None, None, None, 0, 0.9, 0.999, 1e-8, 0.0, None, s) == 0
    assert L.fiber_ema_multi_f32(None, None, None, 0, 0.5, s) == 0
    assert L.fiber_solver_finalize(None, 0, 0.0, None, None, None, 0, 0.9, 0.999, P(block), s) == 1          # max_norm must be positive
    assert L.fiber_solver_finalize(None, 0, 1.0, None, None, None, 0, 0.9, 0.999, None, s) == 1
    assert L.fiber_solver_finalize(None, 0, 1.0, None, None, None, 0, 0.9, 0.999, P(block), s) == 0          # no gradient at all: norm 0, c = 1
    torch.cuda.synchronize()
    assert block.tolist()[2:] == [0, 0] and float(block[1:2].view(torch.float32)) == 1.0 and float(block[0:1].view(torch.float32)) == 0.0


# ---- FiberTorchAdamW ---------------------------------------------------------------------------------------------------------------------------
SHAPES = [(5,), (4097,), (3, 2733), (3,)]
HYPER = [(1e-3, 0.05), (2e-4, 0.0), (5e-4, 0.0125), (1e-3, 0.1)]
ADAM = dict(b1=0.9, b2=0.999, eps=1e-8, d=0.999)


def _groups(params):
    return [{"params": [p], "lr": lr, "weight_decay": wd} for p, (lr, wd) in zip(params, HYPER)]


def _rand(seed, scale=1.0):
    g_ = torch.Generator().manual_seed(seed)
    return [(torch.randn(s, generator=g_) * scale).to(DEV) for s in SHAPES]


def _check_fiber_step(opt, before, grads, t_after, tag):
    """one FiberTorchAdamW step from `before` = [(p, m, v)] fp32 host copies with `grads`: coefficient rows against the closed form for the
    counts t_after, m', v', p' against fp64 within the bounds (from the stored c and rows)"""
    tab = opt._tab
    c = float(opt.clip_coef)
    coef = tab["coef"].cpu().numpy().astype(np.float64)
    params = [p for g in opt.param_groups for p in g["params"] if p.grad is not None]
    for i, (p, (p0, m0, v0), g, t) in enumerate(zip(params, before, grads, t_after)):
        lr, wd = (sc.f32(x) for x in HYPER[i])
        want = np.array([1.0 - lr * wd, lr / (1.0 - sc.f32(0.9) ** t), 1.0 / np.sqrt(1.0 - sc.f32(0.999) ** t)])
        assert np.all(np.abs(coef[i, :3] - want) <= sc.SCALAR_REL * np.abs(want)), (tag, i, coef[i], want)
        st = dict(g=g.cpu().numpy().reshape(-1), m=m0.reshape(-1), v=v0.reshape(-1))
        m1, v1, tm, tv = sc.moments_reference(ADAM, st, c)
        got_m, got_v = (opt.state[p][k].cpu().numpy().reshape(-1) for k in ("exp_avg", "exp_avg_sq"))
        p1, tp = sc.param_reference(ADAM, p0.reshape(-1), got_m.astype(np.float64), got_v.astype(np.float64), coef[i])
        for kind, got, ref, term in (("M", got_m, m1, tm), ("V", got_v, v1, tv), ("P", p.detach().cpu().numpy().reshape(-1), p1, tp)):
            assert_elementwise(f"{tag} tensor {i} {kind}", T64(got), T64(ref), T64(sc.K[kind] * sc.F32 * term + sc.TINY32))


def test_interoperates_with_torch_adamw_state(lib):
    from fiber_amd.optim import FiberTorchAdamW
    tp = [torch.nn.Parameter(t) for t in _rand(1)]
    topt = torch.optim.AdamW(_groups(tp), lr=1e-3)
    for k in range(2):
        for p, g in zip(tp, _rand(10 + k, 0.1)):
            p.grad = g
        topt.step()
    fp = [torch.nn.Parameter(p.detach().clone()) for p in tp]
    fopt = FiberTorchAdamW(_groups(fp), lr=1e-3)
    fopt.load_state_dict(copy.deepcopy(topt.state_dict()))       # (load_state_dict keeps tensors of the right dtype and device as they are)
    before = [(p.detach().cpu().numpy(), fopt.state[p]["exp_avg"].cpu().numpy(), fopt.state[p]["exp_avg_sq"].cpu().numpy()) for p in fp]
    g3 = _rand(12, 0.1)
    for p, g in zip(fp, g3):
        p.grad = g
    fopt.step()
    torch.cuda.synchronize()
    assert float(fopt.clip_coef) == 1.0 and int(fopt.skipped_steps) == 0
    want_norm = float(torch.linalg.vector_norm(torch.cat([g.double().reshape(-1) for g in g3])))
    assert abs(float(fopt.grad_norm) - want_norm) <= sc.SCALAR_REL * want_norm
    _check_fiber_step(fopt, before, g3, [3] * 4, "continued")
    # ... and against torch's own third step: a looser, independent statement of the same (its fp32 arithmetic is another order)
    for p, g in zip(tp, g3):
        p.grad = g.clone()
    topt.step()
    for p, q in zip(fp, tp):
        assert float((p.detach() - q.detach()).abs().max()) <= 1e-5 * float(q.detach().abs().max())
    sd = fopt.state_dict()
    assert [float(s["step"]) for s in sd["state"].values()] == [3.0] * 4 and all(s["step"].dtype == torch.float32 and not s["step"].is_cuda for s in sd["state"].values())
    assert [(g["lr"], g["weight_decay"]) for g in sd["param_groups"]] == HYPER
    back = torch.optim.AdamW(_groups([torch.nn.Parameter(p.detach().clone()) for p in fp]), lr=1e-3)
    back.load_state_dict(copy.deepcopy(sd))
    for (p, q) in zip(back.param_groups, fopt.param_groups):
        a, b = back.state[p["params"][0]], fopt.state[q["params"][0]]
        assert float(a["step"]) == 3.0 and torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])
    for g_, g in zip(back.param_groups, g3):
        g_["params"][0].grad = g.clone()
    back.step()
    assert all(float(back.state[g_["params"][0]]["step"]) == 4.0 for g_ in back.param_groups)


def test_a_parameter_that_joins_late_has_its_own_count(lib):
    from fiber_amd.optim import FiberTorchAdamW
    fp = [torch.nn.Parameter(t) for t in _rand(2)]
    opt = FiberTorchAdamW(_groups(fp), lr=1e-3, max_grad_norm=0.05)
    g1, g2 = _rand(20, 0.1), _rand(21, 0.1)
    for p, g in zip(fp[:3], g1):
        p.grad = g
    opt.step()
    late0 = fp[3].detach().clone()
    assert opt.rebuilds == 1 and not opt.state[fp[3]]
    before = [(p.detach().cpu().numpy(), opt.state[p]["exp_avg"].cpu().numpy(), opt.state[p]["exp_avg_sq"].cpu().numpy()) for p in fp[:3]]
    before.append((late0.cpu().numpy(), np.zeros(3, np.float32), np.zeros(3, np.float32)))
    for p, g in zip(fp, g2):
        p.grad = g
    opt.step()
    torch.cuda.synchronize()
    assert opt.rebuilds == 2 and 0.0 < float(opt.clip_coef) < 1.0
    assert [int(opt.state[p]["step"]) for p in fp] == [2, 2, 2, 1]
    assert [float(s["step"]) for s in opt.state_dict()["state"].values()] == [2.0, 2.0, 2.0, 1.0]
    _check_fiber_step(opt, before, g2, [2, 2, 2, 1], "late")
    opt.step()                                                    # same gradients, same membership: no rebuild, no upload of anything
    assert opt.rebuilds == 2 and [int(opt.state[p]["step"]) for p in fp] == [3, 3, 3, 2]


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(70, 60)                        # 4200 weights: more than a chunk
        self.norm = torch.nn.LayerNorm(60)
        self.frozen = torch.nn.Linear(3, 3)
        self.frozen.requires_grad_(False)
        self.register_buffer("position_ids", torch.arange(7))
        self.register_buffer("scale", torch.ones(3))


def test_model_ema_on_the_device_attached_and_alone(lib):
    """unattached: one launch over every floating entry; attached: the optimizer writes the stepped parameters' EMA, update() the rest.  Both
    equal the fp32-rounded closed form within the EMA bound; integer buffers are copied; version counters of what update() wrote move."""
    from fiber_amd.optim import FiberTorchAdamW
    from fiber_amd.solver import ModelEma
    for attached in (False, True):
        torch.manual_seed(4)
        model = _Tiny().to(DEV)
        ema = ModelEma(model, 0.999)
        assert not ema.ema.training and not any(p.requires_grad for p in ema.ema.parameters())
        opt = FiberTorchAdamW([{"params": [p], "lr": 1e-2, "weight_decay": 0.01} for p in model.parameters() if p.requires_grad], lr=1e-2)
        if attached:
            opt.attach_ema(ema)
        e_prev = {k: v.detach().cpu().numpy().copy() for k, v in ema.state_dict().items()}
        v0 = ema.ema.frozen.weight._version
        for it in range(2):
            model.zero_grad(set_to_none=True)
            model.norm(model.fc(torch.randn(4, 70, device=DEV))).square().sum().backward()
            with torch.no_grad():
                model.position_ids.add_(100003)
                model.scale.mul_(1.5)
            opt.step()
            ema.update(model)
            torch.cuda.synchronize()
            for k, e in ema.state_dict().items():
                cur = model.state_dict()[k].cpu().numpy()
                if e.is_floating_point():
                    ref, term = sc.ema_reference(dict(d=0.999), e_prev[k].reshape(-1), cur.reshape(-1))
                    assert_elementwise(f"attached={attached} it {it} {k}", T64(e.cpu().numpy()), T64(ref), T64(sc.K["EMA"] * sc.F32 * term + sc.TINY32))
                else:
                    assert np.array_equal(e.cpu().numpy(), cur), k
                e_prev[k] = e.detach().cpu().numpy().copy()
        assert ema.ema.frozen.weight._version > v0


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------
WATCHED = {"fusion_backbone.backbone.fpn.fpn_inner2.weight": 1e-4, "fusion_backbone.backbone.body.patch_embed.proj.bias": 1e-4,
           "fusion_backbone.language_backbone.body.model.embeddings.word_embeddings.weight": 1e-5}      # name -> base lr under solver_cfg()
WARMUP = [0.001, 0.25075, 0.5005, 0.75025]


def solver_cfg():
    clip = ns(ENABLED=True, CLIP_VALUE=0.01, CLIP_TYPE="full_model", NORM_TYPE=2.0)
    return ns(OPTIMIZER="ADAMW", BASE_LR=1e-4, LANG_LR=1e-5, BACKBONE_BODY_LR_FACTOR=0.5, BIAS_LR_FACTOR=2, WEIGHT_DECAY=0.05, WEIGHT_DECAY_BIAS=0.0,
              WEIGHT_DECAY_NORM_FACTOR=0.25, MODEL_EMA=0.999, MAX_ITER=100, STEPS=(6, 8), GAMMA=0.1, WARMUP_ITERS=4, WARMUP_FACTOR=0.001,
              WARMUP_METHOD="linear", CLIP_GRADIENTS=clip)


def _detect(model, images, tok):
    model.eval()
    with torch.no_grad():
        return model((images, [(64, 96), (60, 90)]), positive_map={1: [1, 2], 2: [4], 3: 7}, tokenizer_input=tok)


@pytest.fixture(scope="module")
def trained(lib):
    """the detector of test_hip_fpn.py, three GroundingSolver steps; everything the tests below look at, recorded once"""
    from fiber_amd.modules import GeneralizedVLRCNN
    from fiber_amd.modules.grounding_train import pack_targets
    from fiber_amd.optim import FiberTorchAdamW
    from fiber_amd.solver import GroundingSolver
    torch.manual_seed(0)
    cfg = fc.model_cfg()
    cfg.SOLVER = solver_cfg()
    model = GeneralizedVLRCNN(cfg).to(DEV)
    g = np.random.default_rng(0)
    B, T = 2, 256
    images = torch.from_numpy(g.standard_normal((B, 3, 64, 96)).astype(np.float32)).to(DEV)
    ids = torch.from_numpy(g.integers(3, 50000, size=(B, T))).to(DEV)
    am = torch.zeros((B, T), dtype=torch.int64)
    am[0, :9], am[1, :14] = 1, 1
    ids[am.to(DEV) == 0] = 1
    pm = torch.zeros((3, T), dtype=torch.uint8)
    pm[0, 1:3], pm[1, 4], pm[2, 2:5] = 1, 1, 1
    targets = pack_targets([torch.tensor([[8.0, 6.0, 60.0, 50.0], [40.0, 20.0, 90.0, 60.0]]), torch.tensor([[10.0, 10.0, 80.0, 55.0]])],
                           [torch.tensor([1, 2]), torch.tensor([1])], pm, device=DEV)
    tok = {"input_ids": ids, "attention_mask": am.to(DEV)}
    solver = GroundingSolver(cfg, model)
    assert isinstance(solver.optimizer, FiberTorchAdamW) and len(solver.optimizer.param_groups) == 458 and solver.optimizer.max_grad_norm == 0.01
    ema = solver.model_ema
    _detect(ema.ema, images, tok)                                # the EMA model's bf16 working copies are cached from here on
    named = dict(model.named_parameters())
    group_of = {id(gr["params"][0]): gr for gr in solver.optimizer.param_groups}
    run = dict(cfg=cfg, model=model, solver=solver, images=images, tok=tok, targets=targets, snaps=[{k: p.detach().clone() for k, p in named.items()}],
               ints0={k: v.clone() for k, v in model.state_dict().items() if not v.is_floating_point()},
               ema0={k: v.detach().clone() for k, v in ema.ema.named_parameters()}, losses=[], norm=[], norm_ref=[], c=[], lrs=[], had_grad=set())
    for it in range(3):
        model.train()
        run["lrs"].append({k: group_of[id(named[k])]["lr"] for k in WATCHED})
        out = solver.step(model(images, targets=targets, tokenizer_input=tok))
        run["losses"].append({k: float(v) for k, v in out.items()})
        grads = [p.grad.double().reshape(-1) for p in named.values() if p.grad is not None]
        run["had_grad"] |= {k for k, p in named.items() if p.grad is not None}
        run["norm_ref"].append(float(torch.linalg.vector_norm(torch.cat(grads))))
        run["norm"].append(float(solver.optimizer.grad_norm))
        run["c"].append(float(solver.optimizer.clip_coef))
        run["snaps"].append({k: p.detach().clone() for k, p in named.items()})
    run["skipped"] = int(solver.optimizer.skipped_steps)
    return run


def test_grounding_solver_three_steps(trained):
    r = trained
    print("losses", r["losses"], "norm", r["norm"], "c", r["c"])
    assert all(np.isfinite(v) for d in r["losses"] for v in d.values()) and set(r["losses"][0]) == {"loss_reg", "loss_centerness", "loss_cls", "loss_dot_product_token"}
    assert r["skipped"] == 0 and all(0.0 < c <= 1.0 for c in r["c"]) and min(r["c"]) < 1.0
    for got, want in zip(r["norm"], r["norm_ref"]):
        assert abs(got - want) <= sc.SCALAR_REL * want, (got, want)
    p0, p3 = r["snaps"][0], r["snaps"][3]
    named = dict(r["model"].named_parameters())
    still = [k for k in r["had_grad"] if torch.equal(p0[k], p3[k])]
    assert not still, still[:8]
    quiet = [k for k in named if k not in r["had_grad"]]
    assert len(quiet) > 2 and all(k.startswith("rpn.head.cls_logits.") or any(f".encoder.layer.{i}." in k for i in (6, 7, 8, 9)) for k in quiet), quiet[:8]
    assert all(torch.equal(p0[k], p3[k]) for k in quiet)
    for it in range(3):
        for k, base in WATCHED.items():
            assert r["lrs"][it][k] == pytest.approx(base * WARMUP[it], rel=1e-12), (it, k)
    assert r["solver"].scheduler.last_epoch == 3


def test_ema_follows_the_closed_form(trained):
    """ema_3 = d (d (d ema_0 + (1-d) p_1) + (1-d) p_2) + (1-d) p_3 in fp64 from the recorded snapshots; each step's own bound 6 x 2^-24 x
    (|d ema| + |(1-d) p|), carried forward by d per later step"""
    r = trained
    d = float(np.float32(0.999))
    omd = float(np.float32(1) - np.float32(0.999))
    ema_params = dict(r["solver"].model_ema.ema.named_parameters())
    worst = 0.0
    for k, e0 in r["ema0"].items():
        assert torch.equal(e0, r["snaps"][0][k])
        e, bound = e0.double(), torch.zeros_like(e0, dtype=torch.float64)
        for it in range(1, 4):
            a, b = d * e, omd * r["snaps"][it][k].double()
            e, bound = a + b, d * bound + sc.K["EMA"] * sc.F32 * (a.abs() + b.abs()) + sc.TINY32
        worst = max(worst, assert_elementwise(f"ema {k}", ema_params[k].double().reshape(-1, 1), e.reshape(-1, 1), bound.reshape(-1, 1)))
    print(f"ema: worst |err| / bound {worst:.3f}")
    esd = r["solver"].model_ema.state_dict()
    ints = [k for k, v in esd.items() if not v.is_floating_point()]
    assert len(ints) == 9 and all(torch.equal(esd[k], r["ints0"][k]) and esd[k].dtype == r["ints0"][k].dtype for k in ints)


def test_ema_model_does_not_run_on_stale_copies(trained):
    """the EMA model ran before the three steps, so its bf16 working copies were cached; its detections now are, to the bit, those of a
    freshly built model loaded from ema.state_dict()"""
    from fiber_amd.modules import GeneralizedVLRCNN
    r = trained
    ema = r["solver"].model_ema
    got = _detect(ema.ema, r["images"], r["tok"])
    fresh = GeneralizedVLRCNN(r["cfg"]).to(DEV)
    fresh.load_state_dict(ema.state_dict())
    want = _detect(fresh, r["images"], r["tok"])
    for f in ("boxes", "scores", "labels", "count"):
        assert torch.equal(getattr(got, f), getattr(want, f)), f


def test_solver_step_does_not_synchronise(trained):
    """a steady-state step: one unguarded step first, so that the weight-copy tables of ops.py (rebuilt, with a blocking upload, whenever the
    set of cached copies changes -- the model of the test above has just come and gone) are in place"""
    import gc
    r = trained
    model, solver = r["model"], r["solver"]
    gc.collect()
    model.train()
    mode = torch.cuda.get_sync_debug_mode()
    for guarded in (False, True):
        losses = model(r["images"], targets=r["targets"], tokenizer_input=r["tok"])
        rebuilds = solver.optimizer.rebuilds
        if guarded:
            torch.cuda.set_sync_debug_mode("error")
        try:
            out = solver.step(losses)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        assert solver.optimizer.rebuilds == rebuilds              # the tables of the first step still serve
    assert all(bool(torch.isfinite(v)) for v in out.values()) and int(solver.optimizer.skipped_steps) == 0
