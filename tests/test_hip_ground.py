"""GPU tests of the grounding head: csrc/ground.hip through fiber_amd/lib.py and ops, element by element against the fp64 restatement of
tests/ground_cases.py (bounds and their derivation there), bitwise repeatability, VLDyHead against the reference-run fixture
tests/golden/ground_small.npz, fused against plain path, and the memory condition that defines "fused".
FIBER_GROUND_CALIBRATE=<file> writes, per constant of ground_cases.CONST, the largest value any element needed."""
import json
import os

import numpy as np
import pytest
import torch

import ground_cases as gc
from hip_util import assert_elementwise

pytestmark = pytest.mark.gpu
DEV = "cuda"
_CAL = os.environ.get("FIBER_GROUND_CALIBRATE")
_needed = {}


def _note(key, value):
    _needed[key] = max(_needed.get(key, 0.0), float(value))
    if _CAL:
        with open(_CAL, "w") as f:
            json.dump({k: [v, f"2^{np.log2(v):.2f}" if v > 0 else "0"] for k, v in _needed.items()}, f, indent=1)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from fiber_amd import lib
    lib.load()
    return lib


def _dev(case):
    return {k: v.to(DEV) for k, v in case.items()}


def _fwd(lib, c, alpha, gamma, want_logits, want_loss):
    B, A, _ = c["x"].shape
    logits = torch.full((B, A, gc.T), float("nan"), device=DEV) if want_logits else None
    loss = torch.full((), float("nan"), device=DEV) if want_loss else None
    ws = torch.empty(max(1, lib.plain("fiber_ground_workspace", B, A, gc.T)), device=DEV)
    lib.call("fiber_ground_fwd_bf16", lib.ptr(c["x"]), lib.ptr(c["p"]), lib.ptr(c["tbias"]), lib.ptr(c["log_scale"]),
             lib.ptr(c["targets"]) if want_loss else None, lib.ptr(c["mask"]) if want_loss else None, lib.ptr(logits), lib.ptr(loss),
             lib.ptr(ws) if want_loss else None, B, A, gc.T, gc.C, alpha, gamma)
    return logits, loss


def _bwd(lib, c, alpha, gamma, g):
    B, A, _ = c["x"].shape
    ds = torch.full((B, A, gc.T), float("nan"), dtype=torch.bfloat16, device=DEV)
    dtb = torch.full((B, gc.T), float("nan"), device=DEV)
    dls = torch.full((1,), float("nan"), device=DEV)
    ws = torch.empty(lib.plain("fiber_ground_workspace", B, A, gc.T), device=DEV)
    gt = torch.tensor([g], dtype=torch.float32, device=DEV)
    lib.call("fiber_ground_bwd_bf16", lib.ptr(c["x"]), lib.ptr(c["p"]), lib.ptr(c["tbias"]), lib.ptr(c["log_scale"]), lib.ptr(c["targets"]),
             lib.ptr(c["mask"]), lib.ptr(gt), lib.ptr(ds), lib.ptr(dtb), lib.ptr(dls), lib.ptr(ws), B, A, gc.T, gc.C, alpha, gamma)
    return ds, dtb, dls


def _check_sum(name, got, ref, absum, key="SUM"):
    got, ref, absum = got.double().reshape(-1).cpu(), ref.double().reshape(-1).cpu(), absum.double().reshape(-1).cpu()
    err = (got - ref).abs()
    need = float((err / absum.clamp_min(1e-300)).max())
    print(f"{name}: needs {key} {need:.3e}")
    _note(key, need)
    assert bool((err <= gc.CONST[key] * absum).all()), f"{name}: needs {need:.3e} (2^{np.log2(max(need, 1e-300)):.2f}) > {gc.CONST[key]:.3e}"


KERNEL_CASES = {
    "small": dict(B=2, A=gc.A_SMALL, empty_image=1),
    "tail1": dict(B=2, A=1), "tail15": dict(B=2, A=15), "tail129": dict(B=2, A=129),
    "full": dict(B=2, A=gc.A_FULL),
}
HYPER = {"small": [(0.25, 2.0), (-1.0, 1.5), (0.25, 0.0)], "full": [(0.25, 2.0)]}


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_kernel_against_fp64(lib, name):
    c = _dev(gc.kernel_case(name, **KERNEL_CASES[name]))
    if name == "small":                                   # rows that reach the clamp on both sides, one of them a positive
        c["tbias"][0, 5], c["tbias"][1, 2] = 6.0e4, -7.0e4
        c["targets"][0, 9, 5] = 1
    g = 0.37
    for alpha, gamma in HYPER.get(name, [(0.25, 2.0), (-1.0, 1.5)]):
        r = gc.backward64(c["x"], c["p"], c["tbias"], c["log_scale"], c["targets"], c["mask"], alpha, gamma, g)
        lo, _ = _fwd(lib, c, alpha, gamma, True, False)
        lb, both = _fwd(lib, c, alpha, gamma, True, True)
        _, loss = _fwd(lib, c, alpha, gamma, False, True)
        assert torch.equal(lo, lb) and torch.equal(both, loss), "the logits / loss outputs differ between the kernel's instantiations"
        need = float((((lo.double() - r["s"]).abs() - 2.0 ** -23 * r["s"].abs()).clamp_min(0) / r["mag"].clamp_min(1e-300)).max())
        print(f"{name} a={alpha} g={gamma}: logits need K_ACC {need:.3e}")
        _note("K_ACC", need)
        assert_elementwise(f"{name} logits", lo, r["s"], gc.logit_bound(r["mag"], r["s"]))
        _check_sum(f"{name} loss a={alpha} g={gamma}", loss, r["loss"], r["loss_el"].abs().sum())
        ds, dtb, dls = _bwd(lib, c, alpha, gamma, g)
        at = gc.alpha_t(c["targets"], alpha)
        inv = float(r["inv"])
        need = float((((ds.double() - r["dq"]).abs() - 2.0 ** -8 * r["dq"].abs()).clamp_min(0) / (inv * abs(g) * at)).max())
        print(f"{name} a={alpha} g={gamma}: ds needs DS {need:.3e}")
        _note("DS", need)
        assert_elementwise(f"{name} ds", ds, r["dq"], inv * gc.ds_bound(r["ds"], c["targets"], alpha, g))
        _check_sum(f"{name} dtbias", dtb, r["dtbias"], r["dtbias_abs"])
        _check_sum(f"{name} dlog_scale", dls, r["dlog_scale"], r["dlog_scale_abs"])
        if name == "small":
            assert float(r["ds"][0, :, 5].abs().max()) == 0.0 and float(ds[0, :, 5].float().abs().max()) == 0.0, "clamped column must carry no gradient"


def _leaves(c):
    x = c["x"].clone().requires_grad_()
    p = c["p"].float().requires_grad_()
    tb = c["tbias"].clone().requires_grad_()
    ls = c["log_scale"].clone().requires_grad_()
    return x, p, tb, ls


def _fused_grads(c, alpha, gamma, scale=1.0):
    from fiber_amd import ops
    x, p, tb, ls = _leaves(c)
    loss = ops.ground_token_loss(x, p, tb, ls, c["targets"], c["mask"], alpha, gamma)
    (loss * scale).backward()
    return loss.detach(), x.grad, p.grad, tb.grad, ls.grad


@pytest.mark.parametrize("name", ["small", "tail129"])
def test_ops_gradients_against_fp64(lib, name):
    """ground_token_loss through autograd: dX (bf16) and dP (fp32) from the two GEMMs on the bf16 ds.  Bounds: the ds bound carried
    through the product (sum_t bound_t |p_t|, sum_a bound_a |x_a|) + the bf16 rounding of dX / the fp32 accumulation of dP."""
    c = _dev(gc.kernel_case(name, **KERNEL_CASES[name]))
    alpha, gamma, g = 0.25, 2.0, 0.5
    r = gc.backward64(c["x"], c["p"], c["tbias"], c["log_scale"], c["targets"], c["mask"], alpha, gamma, g)
    loss, dx, dp, dtb, dls = _fused_grads(c, alpha, gamma, g)
    dsb, dqa = r["inv"] * gc.ds_bound(r["ds"], c["targets"], alpha, g), r["dq"].abs()
    pa, xa = c["p"].double().abs(), c["x"].double().abs()
    assert_elementwise(f"{name} dX", dx, r["dx"], torch.matmul(dsb, pa) + 2.0 ** -8 * r["dx"].abs() + gc.CONST["SUM"] * torch.matmul(dqa, pa))
    assert_elementwise(f"{name} dP", dp, r["dp"], torch.matmul(dsb.transpose(1, 2), xa) + gc.CONST["SUM"] * torch.matmul(dqa.transpose(1, 2), xa))
    _check_sum(f"{name} ops dtbias", dtb, r["dtbias"], r["dtbias_abs"])
    _check_sum(f"{name} ops dlog_scale", dls, r["dlog_scale"], r["dlog_scale_abs"])


def test_two_runs_bitwise(lib):
    c = _dev(gc.kernel_case("full", **KERNEL_CASES["full"]))
    a = _fused_grads(c, 0.25, 2.0)
    b = _fused_grads(c, 0.25, 2.0)
    for n, u, v in zip(("loss", "dX", "dP", "dtbias", "dlog_scale"), a, b):
        assert torch.equal(u, v), f"{n}: two runs differ"


def _torch_loss(s, tg, mask, alpha, gamma):
    from fiber_amd.modules.vldyhead import TokenSigmoidFocalLoss
    return TokenSigmoidFocalLoss(alpha, gamma)(s, tg, mask)


def test_fused_equals_plain(lib):
    from fiber_amd import ops
    c = _dev(gc.kernel_case("small", **KERNEL_CASES["small"]))
    alpha, gamma = 0.25, 2.0
    r = gc.backward64(c["x"], c["p"], c["tbias"], c["log_scale"], c["targets"], c["mask"], alpha, gamma, 1.0)
    fl, fdx, fdp, fdtb, fdls = _fused_grads(c, alpha, gamma)
    x, p, tb, ls = _leaves(c)
    pl = _torch_loss(ops.ground_logits(x, p, tb, ls), c["targets"], c["mask"], alpha, gamma)
    pl.backward()
    absum = r["loss_el"].abs().sum()
    assert abs(float(fl) - float(pl)) <= 2 * gc.CONST["SUM"] * float(absum), (float(fl), float(pl))
    dsb = r["inv"] * gc.ds_bound(r["ds"], c["targets"], alpha, 1.0)
    pa, xa = c["p"].double().abs(), c["x"].double().abs()
    assert_elementwise("fused vs plain dX", fdx, x.grad, 2 * (torch.matmul(dsb, pa) + 2.0 ** -8 * r["dx"].abs()))
    assert_elementwise("fused vs plain dP", fdp, p.grad, 2 * (torch.matmul(dsb.transpose(1, 2), xa) + gc.CONST["SUM"] * torch.matmul(r["dq"].abs().transpose(1, 2), xa)))
    assert_elementwise("fused vs plain dtbias", fdtb, tb.grad, 2 * gc.CONST["SUM"] * r["dtbias_abs"] + 1e-30)
    assert abs(float(fdls) - float(ls.grad)) <= 2 * gc.CONST["SUM"] * float(r["dlog_scale_abs"])


def test_empty_targets_and_default_mask(lib):
    from fiber_amd import ops
    c = _dev(gc.kernel_case("tail15", **KERNEL_CASES["tail15"]))
    assert float(ops.ground_token_loss(c["x"][:, :0], c["p"], c["tbias"], c["log_scale"], c["targets"][:, :0], None)) == 0.0
    ones = torch.ones_like(c["mask"])
    a = ops.ground_token_loss(c["x"], c["p"], c["tbias"], c["log_scale"], c["targets"].float(), None, 0.25, 2.0)
    b = ops.ground_token_loss(c["x"], c["p"], c["tbias"], c["log_scale"], c["targets"], ones, 0.25, 2.0)
    assert torch.equal(a, b)
    with pytest.raises(lib.FiberHipError):                # T = 128: only C = T = 256 is built
        lib.call("fiber_ground_fwd_bf16", lib.ptr(c["x"]), lib.ptr(c["p"]), lib.ptr(c["tbias"]), lib.ptr(c["log_scale"]), None, None,
                 lib.ptr(torch.empty((2, 15, 128), device=DEV)), None, None, 2, 15, 128, gc.C, -1.0, 0.0)


def test_memory_condition(lib):
    """"Fused" as a condition: at B = 2, A = 22 400 the forward of ground_token_loss raises the peak by less than ONE [B, A, T] fp32
    tensor and forward + backward by less than TWO; the plain-torch statement of the same lines exceeds both."""
    from fiber_amd import ops
    c = _dev(gc.kernel_case("full", **KERNEL_CASES["full"]))
    one = 2 * gc.A_FULL * gc.T * 4
    alpha, gamma = 0.25, 2.0

    def peak(fn):
        leaves = _leaves(c)                               # the caller's own tensors are not the operator's memory
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn(*leaves)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
        del out, leaves
        return rise

    def fused_fwd(x, p, tb, ls):
        return ops.ground_token_loss(x, p, tb, ls, c["targets"], c["mask"], alpha, gamma)

    def fused_both(x, p, tb, ls):
        ops.ground_token_loss(x, p, tb, ls, c["targets"], c["mask"], alpha, gamma).backward()
        return x.grad, p.grad

    def plain(backward, x, p, tb, ls):
        s = (torch.matmul(x.float(), p.transpose(-1, -2)) / ls.exp() + tb.unsqueeze(1).repeat(1, x.shape[1], 1)).clamp(max=50000).clamp(min=-50000)
        m = (c["mask"] > 0).unsqueeze(1).repeat(1, s.size(1), 1)
        lg, tg = torch.masked_select(s, m), torch.masked_select(c["targets"].float(), m)
        pr = torch.sigmoid(lg)
        ce = torch.nn.functional.binary_cross_entropy_with_logits(lg, tg, reduction="none")
        p_t = pr * tg + (1 - pr) * (1 - tg)
        loss = ((alpha * tg + (1 - alpha) * (1 - tg)) * (ce * ((1 - p_t) ** gamma))).sum()
        if backward:
            loss.backward()
        return loss

    f1, f2, t1, t2 = peak(fused_fwd), peak(fused_both), peak(lambda *l: plain(False, *l)), peak(lambda *l: plain(True, *l))
    print(f"peak rise in units of one [B, A, T] fp32 tensor: fused fwd {f1 / one:.3f}, fused fwd+bwd {f2 / one:.3f}, torch fwd {t1 / one:.2f}, torch fwd+bwd {t2 / one:.2f}")
    assert f1 < one, f"fused forward raises the peak by {f1 / one:.3f} tensors"
    assert f2 < 2 * one, f"fused forward + backward raises the peak by {f2 / one:.3f} tensors"
    assert t1 > one and t2 > 2 * one, (t1 / one, t2 / one)


# ---- the module against the reference-run fixture -------------------------------------------------------------------------------------
# measured on MI355X against tests/golden/ground_small.npz; next power of two at or above the observed value (in brackets).  The differences
# are the tower's: bf16 activations and GEMM operands against the reference's fp32 run (the deformable sampling of both sides is
# oracle/dcn_ref.py's formulation).
MODULE_TOL = {
    "loss": 2.0 ** -13,         # relative (9.35e-5)
    "grad_norm": 2.0 ** -6,     # relative, every parameter (1.204e-2)
    "named_grad": 2.0 ** -9,    # rel-L2 of log_scale, bias0, bias_lang, dot_product_projection_text.weight, d embedding (1.642e-3, the weight)
    "dx": 2.0 ** -4,            # rel-L2 per level, through two deformable layers' offsets (4.84e-2, level 0); norms 1.6e-3
    "heads": 2.0 ** -7,         # rel-L2 of cls / box / centerness maps (6.13e-3, cls level 0)
}


def _head():
    from fiber_amd.modules import VLDyHead
    m = VLDyHead(gc.head_cfg(convs=gc.SMALL["convs"]))
    gc.set_head_weights(m)
    return m.to(DEV)


def test_head_forward_against_reference(lib, golden):
    gold = golden("ground_small")
    m = _head()
    xs, emb, tg, mask = gc.small_inputs()
    with torch.no_grad():
        out = m([x.to(DEV) for x in xs], None, emb.to(DEV))
    assert len(out) == 10 and all(out[i] is None for i in (3, 4, 5, 7, 8, 9))
    rows = gold["rows"]
    for l in range(len(xs)):
        for k, t in (("logits", out[0][l]), ("bbox_reg", out[1][l]), ("centerness", out[2][l])):
            ref = torch.from_numpy(gold[f"{k}{l}"])
            e = gc.rel_l2(t.cpu(), ref)
            print(f"{k}{l}: rel-L2 {e:.3e}")
            assert e <= MODULE_TOL["heads"], (k, l, e)
        assert out[6][l].shape == (gc.SMALL["B"], xs[l].shape[2] * xs[l].shape[3], gc.T)
    got = torch.cat(out[6], dim=1).cpu()[:, rows]
    e = gc.rel_l2(got, torch.from_numpy(gold["dot_rows"]))
    print(f"dot_product_logits (sampled rows): rel-L2 {e:.3e}")
    # operand rounding (tower features and projected tokens rounded to bf16 by us, not by the reference): 2^-8 sum_k |x_k p_k| inv_scale
    bound = (2.0 ** -8 + gc.CONST["K_ACC"]) * torch.from_numpy(gold["dot_mag_rows"]).double() + 2.0 ** -23 * torch.from_numpy(gold["dot_rows"]).double().abs()
    tower_err = torch.from_numpy(gold["dot_rows"]).double().sub(got.double()).abs()
    worst = float((tower_err / bound).max())
    print(f"dot_product_logits: worst |err| / bound {worst:.3f}")               # 0.551 on MI355X
    assert worst <= 1.0, f"dot_product_logits: {worst:.3f} x the operand-rounding bound"


def test_head_token_loss_against_reference(lib, golden):
    gold = golden("ground_small")
    m = _head()
    xs, emb, tg, mask = gc.small_inputs()
    xs = [x.to(DEV).requires_grad_() for x in xs]
    emb = emb.to(DEV).requires_grad_()
    loss = m.token_loss(xs, emb, tg.to(DEV), mask.to(DEV), gc.SMALL["num_pos"], gc.SMALL["alpha"], gc.SMALL["gamma"])
    loss.backward()
    e = abs(float(loss) - float(gold["loss"])) / abs(float(gold["loss"]))
    print(f"loss {float(loss):.6f} reference {float(gold['loss']):.6f} rel {e:.3e}")
    assert e <= MODULE_TOL["loss"]
    for l, x in enumerate(xs):
        e = gc.rel_l2(x.grad.cpu()[:, gold["chans"]], torch.from_numpy(gold[f"dx{l}"]))
        en = abs(float(x.grad.norm()) - float(gold[f"dx_norm{l}"])) / float(gold[f"dx_norm{l}"])
        print(f"dx{l}: rel-L2 {e:.3e}, norm rel {en:.3e}")
        assert e <= MODULE_TOL["dx"] and en <= MODULE_TOL["dx"], (l, e, en)
    e = gc.rel_l2(emb.grad.cpu()[:, :gc.KEEP_TOKENS], torch.from_numpy(gold["dembedding"]))
    en = abs(float(emb.grad.norm()) - float(gold["dembedding_norm"])) / float(gold["dembedding_norm"])
    print(f"dembedding: rel-L2 {e:.3e}, norm rel {en:.3e}")
    assert e <= MODULE_TOL["named_grad"] and en <= MODULE_TOL["named_grad"]
    params = dict(m.named_parameters())
    for k in ("log_scale", "bias0", "bias_lang", "dot_product_projection_text.weight"):
        got = params[k].grad.cpu()
        e = gc.rel_l2(got[gold["wrows"]] if k.endswith(".weight") else got, torch.from_numpy(gold["grad:" + k]))
        print(f"grad {k}: rel-L2 {e:.3e}")
        assert e <= MODULE_TOL["named_grad"], (k, e)
    worst = 0.0
    for k, n in zip(gold["param_names"], gold["grad_norms"]):
        p = params[str(k)]
        if n == 0.0:
            assert p.grad is None or float(p.grad.norm()) == 0.0, k
            continue
        worst = max(worst, abs(float(p.grad.norm()) - n) / n)
    print(f"parameter gradient norms: worst relative difference {worst:.3e}")
    assert worst <= MODULE_TOL["grad_norm"]
