"""Case table of the grounding side of the autograd layer (fiber_amd/ops.py): _DeformConv, _Conv1x1, _FpnMerge, _GroundLogits,
_GroundTokenLoss and _AtssBoxLosses at the smallest shapes that reach each branch of their backward, with the plain operation in torch
fp64 autograd as the reference.  The machinery (Case / Entry, leaves_of, subsets, reference, needed, plain_mid, backward, the bound) is
that of tests/autograd_cases.py; the kernels themselves are pinned per element at the C ABI by dcn_cases / ground_cases / atss_cases /
fpn_cases, whose bounds are taken unchanged where a Function adds nothing to its kernel.  Shared by
tests/test_hip_ground_autograd_graphs.py (the Functions on the GPU under the graph variants (a) to (f)) and
tests/test_ground_autograd_host.py (references, twins and bounds on the host).

Bound, per element (hip_util.assert_elementwise):   |got - ref| <= 2^-8 |ref| + CONST[family] * A + TINY
A is the fp64 absolute twin of a gradient: the same sum over the magnitudes of its factors.  What each twin carries:
  dcn       cols is a bf16 tensor (enters dW), dcols = dY W is a bf16 tensor (enters dx, doffset, dmask), an fp32 incoming gradient
            (out_fp32) is rounded to bf16 before both GEMMs: each at most 2^-8 (half an ulp of bf16 just above a power of two) of
            the products it enters, so A = the product of magnitudes.
            The tiled dx adds n 2^(e - 20) (dcn_cases: n window contributions, 2^e the power of two above max |dcols|), carried as
            n 2^-10 max |dcols|.
  dyconv    as dcn, twice: the gradient of the offset tensor is the fp32 fan-in sum of two doffset / dmask (each with the 2^-8 of its
            dcols), rounded to bf16 by the offset convolution's backward; dx is the bf16 fan-in sum of two bf16 dx.
  conv1x1   nothing beyond fp32 accumulation: x, W, dY are bf16-exact.
  fpn       element-wise fp32 (fpn_cases: at most 2 (n_children + 2) 2^-24 of the terms); in a chain d_coarse is a bf16 tensor that
            enters the coarse level's gradient (2^-8), and a second consumer of `inner` adds the bf16 fan-in sum (its own term).
  ground    ds = d(raw dot product) is a bf16 tensor in front of both GEMMs (2^-8); dtbias and dlog_scale are fp32 sums of the fp32 ds
            (ground_cases SUM, unchanged).
  atss      the Function launches the kernels and nothing else: A is the ABI bound of atss_cases itself, constant 1.

Per entry `branch` names the branch reached and the line of ops.py that selects it (_DeformConv.backward: `tiled = need_x and kh == 3 and
... C % 16 == 0`; the scatter launch runs `if dxf is not None or need_off or need_mask`; db without dW takes `elif need_db`), and
`atomics` the leaves whose gradient passes fp32 atomics: those are compared within the bound under (c) and (f), every other gradient
bitwise.  The only fp32 atomics on these paths are `if (dx) { ... unsafeAtomicAdd ...}` of dcn_scatter_kernel (csrc/dcn.hip), reached
when ops.py passes `dxf` (C % 16 != 0: dcn-c8's dx); the tiled dx adds fixed-point integers in LDS, and its `far` map (fp32 atomics for
corners outside a tile's 24 x 24 window) receives nothing on 5 x 7 and 9 x 13 maps, which lie inside one window.  Everything else is
bitwise because the copy `_c(dy.to(BF16))` (`_c(g.detach().float().reshape(3))` for the ATSS sums) at the head of each backward makes
every form of the incoming gradient the same dense tensor, and no other kernel on these paths accumulates in an order that varies."""
import numpy as np
import torch
import torch.nn.functional as F

import atss_cases
import dcn_cases
import fpn_cases
import ground_cases
from oracle import dcn_ref
from tests import autograd_cases as AC
from tests.autograd_cases import Case, Entry, backward, leaves_of, needed, plain_mid, rn_none, subsets  # noqa: F401  (re-exported)
from tests.hip_util import abs_mm64

BF = torch.bfloat16
# One constant per family, in units of the twin A: the rounding the family performs inside the graph, then the smallest power of two
# variant (a) -- every input live -- needed on the first MI355X run over all entries of the family (test_all_live prints CALIB lines).
# Not to be raised to admit another variant.
CONST = {
    # derived 2^-7: bf16 dcols or cols (2^-8 at worst) + the bf16 rounding of an fp32 incoming gradient (2^-8)
    "dcn": 2.0 ** -9,          # needed 2^-9.29, dcn-c16-s2 dw
    # derived 2^-6: the above through two chained convolutions + the bf16 rounding of the fan-in gradient
    "dyconv": 2.0 ** -10,      # needed 2^-10.004, dyconv dxf (the offset convolution's own wo / bo / x: 2^-13.3 and less)
    "conv1x1": 2.0 ** -20,     # fp32 accumulation only (gemm_cases 2^-20); not calibrated: nothing needed beyond the bf16 store
    "fpn": 2.0 ** -20,         # fpn_cases' ceiling 2 (n_children + 2) 2^-24 <= 12 2^-24, unchanged; not calibrated: nothing needed more
    # derived 2^-8: d_coarse is a bf16 tensor
    "fpn_chain": 2.0 ** -9,    # needed 2^-9.59, fpn-chain dlat_c
    # derived 2^-8: ds is a bf16 tensor
    "ground": 2.0 ** -8,       # needed 2^-8.54, loss-u8-mask dp
    "ground_sum": ground_cases.CONST["SUM"],     # 1 x the ABI bound of the dtbias / dlog_scale sums; nothing needed beyond the store term
    "atss": 2.0 ** 0,          # multiplies the kernel-level bound of atss_cases (K_GRAD 2^-23 magnitude): 1 = the ABI bound unchanged
}
assert not set(CONST) & set(AC.CONST)
AC.CONST.update(CONST)          # AC.bound / AC.reference look a family up there


def _entry(name, family, make, run, ref, twin, branch, atomics=(), leaf_family=None, zeros=None, mid_shape=None):
    e = Entry(name, family, make, run, ref, twin, leaf_family)
    e.branch, e.atomics, e.zeros, e.mid_shape = branch, tuple(atomics), zeros, mid_shape
    return e


def _ident(t):
    return t


# ---- _DeformConv --------------------------------------------------------------------------------------------------------------------
def _conv_ref(x, off, m, w, b, stride, rn, out_fp32=False):
    """oracle/dcn_ref.py's differentiable form on channels-last x [B, H, W, C], off [M, 18] / m [M, 9] or None -> [B, Ho, Wo, Cout].
    rn rounds where the Function stores bf16: cols forward and dcols backward, the result (not with out_fp32) and its gradient."""
    B, H, W, C = x.shape
    Cout = w.shape[0]
    Ho, Wo = dcn_ref._geom(H, W, 3, 3, stride, 1, 1)
    dt = x.dtype
    o4 = off.reshape(B, Ho, Wo, 18).permute(0, 3, 1, 2) if off is not None else torch.zeros(B, 18, Ho, Wo, dtype=dt, device=x.device)
    m4 = m.reshape(B, Ho, Wo, 9).permute(0, 3, 1, 2) if m is not None else torch.ones(B, 9, Ho, Wo, dtype=dt, device=x.device)
    cols = rn(dcn_ref.sample_columns(x.permute(0, 3, 1, 2), o4.to(dt), m4.to(dt), 3, 3, stride, 1))
    y = torch.einsum("oct,bctp->bop", w.to(dt).reshape(Cout, C, 9), cols)
    if b is not None:
        y = y + b.to(dt).view(1, -1, 1)
    return rn(y.view(B, Cout, Ho, Wo).permute(0, 2, 3, 1), fwd=not out_fp32)


def _dcn_twin(x, off, m, w, dy_abs, stride, tiled):
    """Twins of one convolution from dcn_cases.reference (the kernel table's own magnitude sums) with dcols := |dY| |W|:
    {x, w, b[, offset, mask]} on x's device.  dy_abs [.., Cout]: magnitudes of the incoming gradient."""
    B, H, W, C = x.shape
    Cout = w.shape[0]
    c = dcn_cases._case("twin", "tiled", B, H, W, C, stride, off=None if off is None else "given", mask=m is not None)
    wr = w.detach().double().cpu().permute(0, 2, 3, 1).reshape(Cout, 9 * C).abs()
    dya = dy_abs.detach().double().cpu().reshape(-1, Cout)
    dcols = dya @ wr
    f32 = lambda t: None if t is None else t.detach().float().cpu().contiguous().numpy()     # noqa: E731
    r = dcn_cases.reference(c, dict(x=x.detach().double().cpu().numpy(), offset=f32(off), mask=f32(m), dcols=dcols.numpy()))
    A = {"x": torch.from_numpy(r["dx_abs"]), "b": dya.sum(0),
         "w": (dya.t() @ torch.from_numpy(r["cols_abs"])).view(Cout, 3, 3, C).permute(0, 3, 1, 2)}
    if tiled:
        A["x"] = A["x"] + torch.from_numpy(r["n_win"])[..., None] * 2.0 ** -10 * float(dcols.max())
    if off is not None:
        A["offset"], A["mask"] = torch.from_numpy(r["doffset_abs"]), torch.from_numpy(r["dmask_abs"])
    return {k: v.to(x.device) for k, v in A.items()}


def _lattice_offsets(M, g):
    """fp32 [M, 18] on the 1/64 lattice within +-2 px: the kernel's one fp32 addition base + offset is exact, so floor, the `inside`
    test and the corner flags of the fp64 reference agree with the kernels'"""
    return torch.randint(-128, 129, (M, 18), generator=g).float() / 64.0


def _dcn_entry(name, C, Cout, branch, stride=1, deform=True, bias=True, out_fp32=False, atomics=()):
    B, H, W = 2, 5, 7
    Ho, Wo = dcn_ref._geom(H, W, 3, 3, stride, 1, 1)
    M = B * Ho * Wo

    def make(device):
        g = AC._gen(name)
        leaves = [("x", AC._bf((B, H, W, C), g, device))]
        if deform:
            leaves += [("offset", _lattice_offsets(M, g).to(device)), ("mask", torch.sigmoid(torch.randn(M, 9, generator=g) * 2).to(device))]
        leaves.append(("w", AC._f32x((Cout, C, 3, 3), g, device, (9 * C) ** -0.5)))
        if bias:
            leaves.append(("b", AC._f32x((Cout,), g, device, 0.1)))
        gy = AC._randn((B, Ho, Wo, Cout), g, device) if out_fp32 else AC._bf((B, Ho, Wo, Cout), g, device)
        return Case(leaves, ["w"] + (["b"] if bias else []), {}, [gy])

    def run(ops, L, E, mid=plain_mid):
        return (ops.deform_conv(L["x"], L.get("offset"), L.get("mask"), L["w"], L.get("b"), stride=stride, pad=1, out_fp32=out_fp32),)

    def ref(L, E, mid=plain_mid, rn=rn_none):
        return (_conv_ref(L["x"], L.get("offset"), L.get("mask"), L["w"], L.get("b"), stride, rn, out_fp32),)

    def twin(L, E, gs, dmid=None):
        return _dcn_twin(L["x"], L.get("offset"), L.get("mask"), L["w"], gs[0].double().abs(), stride, tiled=C % 16 == 0)

    return _entry(name, "dcn", make, run, ref, twin, branch, atomics)


def _dyconv_entry(name):
    """DyConv's sharing (layers/dyhead.py:93-101): one out_fp32 offset convolution on the map x, its 27 channels split into offset
    and sigmoid(mask) and read by the stride-1 deformable convolution of x and the stride-2 one of the finer map xf.  x feeds the
    offset convolution too: x and the offset tensor both receive a fan-in."""
    B, H, W, C = 2, 5, 7, 16
    Hf, Wf = 9, 13                                                     # stride 2 -> 5 x 7

    def make(device):
        g = AC._gen(name)
        leaves = [("x", AC._bf((B, H, W, C), g, device)), ("xf", AC._bf((B, Hf, Wf, C), g, device)),
                  ("wo", AC._f32x((27, C, 3, 3), g, device, 0.08)), ("bo", AC._f32x((27,), g, device, 0.3))]
        for i in (1, 2):
            leaves += [(f"w{i}", AC._f32x((C, C, 3, 3), g, device, (9 * C) ** -0.5)), (f"b{i}", AC._f32x((C,), g, device, 0.1))]
        return Case(leaves, ["wo", "bo", "w1", "b1", "w2", "b2"], {}, [AC._bf((B, H, W, C), g, device) for _ in range(2)])

    def split(t):
        o2 = t.reshape(-1, 27)
        return o2[:, :18], torch.sigmoid(o2[:, 18:])

    def run(ops, L, E, mid=plain_mid):
        om = ops.deform_conv(L["x"], None, None, L["wo"], L["bo"], out_fp32=True)

        def use(t):
            off, m = split(t)
            return (ops.deform_conv(L["x"], off, m, L["w1"], L["b1"], stride=1), ops.deform_conv(L["xf"], off, m, L["w2"], L["b2"], stride=2))
        return tuple(mid(om, use))

    def ref(L, E, mid=plain_mid, rn=rn_none):
        om = _conv_ref(L["x"], None, None, L["wo"], L["bo"], 1, rn, out_fp32=True)

        def use(t):
            off, m = split(t)
            return (_conv_ref(L["x"], off, m, L["w1"], L["b1"], 1, rn), _conv_ref(L["xf"], off, m, L["w2"], L["b2"], 2, rn))
        return tuple(mid(om, use))

    def twin(L, E, gs, dmid=None):
        z = lambda i: gs[i].double().abs() if gs[i] is not None else torch.zeros(B, H, W, C, dtype=torch.float64, device=L["x"].device)   # noqa: E731
        with torch.no_grad():
            om = _conv_ref(L["x"].double(), None, None, L["wo"].double(), L["bo"].double(), 1, rn_none, out_fp32=True)
        off, m = split(om)
        r1 = _dcn_twin(L["x"], off, m, L["w1"], z(0), 1, True)
        r2 = _dcn_twin(L["xf"], off, m, L["w2"], z(1), 2, True)
        dom = torch.cat([r1["offset"] + r2["offset"], (r1["mask"] + r2["mask"]) * m * (1.0 - m)], 1)
        if dmid is not None:
            dom = dom + dmid.double().abs().reshape(-1, 27)
        r0 = _dcn_twin(L["x"], None, None, L["wo"], dom, 1, True)
        return {"x": r1["x"] + r0["x"], "xf": r2["x"], "wo": r0["w"], "bo": r0["b"], "w1": r1["w"], "b1": r1["b"], "w2": r2["w"], "b2": r2["b"]}

    e = _entry(name, "dyconv", make, run, ref, twin,
               "all three tiled; the offset conv's dy arrives fp32 [.., 27] and is padded to Cp = 32 (`if Cp != Cout`)", mid_shape=(B, H, W, 27))
    e.coords = lambda L: _dyconv_coords(L, split)
    return e


def _dyconv_coords(L, split):
    """distance of every sampling coordinate of the fp64 reference from the nearest integer: where it is below the fp32 rounding of
    the offsets the kernels may floor to the other cell and the gradients are not comparable"""
    with torch.no_grad():
        om = _conv_ref(L["x"].double(), None, None, L["wo"].double(), L["bo"].double(), 1, rn_none, out_fp32=True)
    off, _ = split(om)
    return float((off - torch.round(off)).abs().min())


# ---- _Conv1x1 -----------------------------------------------------------------------------------------------------------------------
def _conv1x1_entry(name, bias, nchw=False):
    shape, N = (2, 3, 5, 16), 24

    def make(device):
        g = AC._gen(name)
        x = AC._bf(shape, g, device)
        if nchw:                                                       # NCHW memory under the channels-last shape
            x = x.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
            assert not x.is_contiguous()
        leaves = [("x", x), ("w", AC._f32x((N, shape[-1], 1, 1), g, device, shape[-1] ** -0.5))] + ([("b", AC._f32x((N,), g, device, 0.1))] if bias else [])
        return Case(leaves, ["w"] + (["b"] if bias else []), {}, [AC._bf(shape[:-1] + (N,), g, device)])

    def run(ops, L, E, mid=plain_mid):
        return (ops.conv1x1(L["x"], L["w"], L.get("b")),)

    def ref(L, E, mid=plain_mid, rn=rn_none):
        dt = L["x"].dtype
        y = F.conv2d(L["x"].permute(0, 3, 1, 2), L["w"].to(dt), L["b"].to(dt) if bias else None)
        return (rn(y.permute(0, 2, 3, 1)),)

    def twin(L, E, gs, dmid=None):
        x, w, dy = AC._rows(L["x"]).double(), L["w"].double().view(N, -1), AC._rows(gs[0]).double()
        return {"x": abs_mm64(dy, w.t()).view(L["x"].shape), "w": abs_mm64(dy.t(), x.t()).view(L["w"].shape), "b": dy.abs().sum(0)}

    return _entry(name, "conv1x1", make, run, ref, twin, "dX on the NT kernel, dW (+ db) on the TN kernel; db alone: `elif need_db: colsum`")


# ---- _FpnMerge ----------------------------------------------------------------------------------------------------------------------
def _keep(name, B, H, W, device):
    g = np.random.default_rng(sum(map(ord, name)))
    kept = 0
    while not 0 < kept < B * H * W:                                    # (a 3 x 5 map may draw no block centre, or drop everything)
        keep, kept = fpn_cases.mask_ref((g.random((B, H, W)) < 0.08).astype(np.uint8), 3)
    return torch.from_numpy(keep).to(device), torch.tensor([kept], dtype=torch.int32, device=device)


def _merge_ref(lat, coarse, keep, kept, rn):
    """F.interpolate(mode="nearest") + the DropBlock scaling of fpn_cases: (inner, dropped or None), dropped from the unrounded sum"""
    s = lat
    if coarse is not None:
        s = s + F.interpolate(coarse.permute(0, 3, 1, 2), size=lat.shape[1:3], mode="nearest").permute(0, 2, 3, 1)
    if keep is None:
        return rn(s), None
    scale = float(keep.numel()) / float(kept)
    return rn(s), rn(s * (keep.to(s.dtype) * scale)[..., None])


def _merge_abs(d_inner, d_dropped, keep, kept, coarse_shape):
    """(A_lateral, A_coarse): |d_inner| + |d_dropped| keep scale, and its sum over the children of every coarse pixel"""
    a = 0.0
    if d_inner is not None:
        a = a + d_inner.double().abs()
    if d_dropped is not None:
        a = a + d_dropped.double().abs() * (keep.double() * (float(keep.numel()) / float(kept)))[..., None]
    if coarse_shape is None or not torch.is_tensor(a):
        return a, None
    c0 = torch.zeros(coarse_shape, dtype=torch.float64, device=a.device, requires_grad=True)
    with torch.enable_grad():
        up = F.interpolate(c0.permute(0, 3, 1, 2), size=a.shape[1:3], mode="nearest").permute(0, 2, 3, 1)
        (ac,) = torch.autograd.grad(up, c0, a)
    return a, ac


def _fpn_entry(name, lat_hw, coarse_hw, with_keep, branch):
    B, C = 2, 16

    def make(device):
        g = AC._gen(name)
        leaves = [("lateral", AC._bf((B,) + lat_hw + (C,), g, device))]
        if coarse_hw:
            leaves.append(("coarse", AC._bf((B,) + coarse_hw + (C,), g, device)))
        E = {}
        if with_keep:
            E["keep"], E["kept"] = _keep(name, B, *lat_hw, device)
        return Case(leaves, [], E, [AC._bf((B,) + lat_hw + (C,), g, device) for _ in range(2 if with_keep else 1)])

    def run(ops, L, E, mid=plain_mid):
        inner, dropped = ops.fpn_merge(L["lateral"], L.get("coarse"), E.get("keep"), E.get("kept"))
        return (inner, dropped) if with_keep else (inner,)

    def ref(L, E, mid=plain_mid, rn=rn_none):
        inner, dropped = _merge_ref(L["lateral"], L.get("coarse"), E.get("keep"), E.get("kept"), rn)
        return (inner, dropped) if with_keep else (inner,)

    def twin(L, E, gs, dmid=None):
        a, ac = _merge_abs(gs[0], gs[1] if with_keep else None, E.get("keep"), E.get("kept"), L["coarse"].shape if coarse_hw else None)
        if not torch.is_tensor(a):
            a = torch.zeros(L["lateral"].shape, dtype=torch.float64, device=L["lateral"].device)
            ac = torch.zeros(L["coarse"].shape, dtype=torch.float64, device=a.device) if coarse_hw else None
        return {"lateral": a, "coarse": ac}

    return _entry(name, "fpn", make, run, ref, twin, branch)


def _fpn_chain_entry(name):
    """Two levels of the top-down chain: the coarse level's `inner` is the fine level's `coarse`, each level's `dropped` goes to the
    loss, the fine `inner` goes nowhere (fpn.py: the finest level is read through its DropBlock only)."""
    B, C, hc, hf = 2, 16, (3, 5), (6, 10)

    def make(device):
        g = AC._gen(name)
        leaves = [("lat_c", AC._bf((B,) + hc + (C,), g, device)), ("lat_f", AC._bf((B,) + hf + (C,), g, device))]
        E = {}
        E["keep_c"], E["kept_c"] = _keep(name + "c", B, *hc, device)
        E["keep_f"], E["kept_f"] = _keep(name + "f", B, *hf, device)
        return Case(leaves, [], E, [AC._bf((B,) + hc + (C,), g, device), AC._bf((B,) + hf + (C,), g, device)])

    def run(ops, L, E, mid=plain_mid):
        inner_c, drop_c = ops.fpn_merge(L["lat_c"], None, E["keep_c"], E["kept_c"])
        return (drop_c, mid(inner_c, lambda t: ops.fpn_merge(L["lat_f"], t, E["keep_f"], E["kept_f"])[1]))

    def ref(L, E, mid=plain_mid, rn=rn_none):
        inner_c, drop_c = _merge_ref(L["lat_c"], None, E["keep_c"], E["kept_c"], rn)
        return (drop_c, mid(inner_c, lambda t: _merge_ref(L["lat_f"], t, E["keep_f"], E["kept_f"], rn)[1]))

    def twin(L, E, gs, dmid=None):
        af, ac = _merge_abs(None, gs[1], E["keep_f"], E["kept_f"], L["lat_c"].shape) if gs[1] is not None else \
            (torch.zeros(L["lat_f"].shape, dtype=torch.float64, device=L["lat_f"].device), torch.zeros(L["lat_c"].shape, dtype=torch.float64, device=L["lat_c"].device))
        if dmid is not None:                                           # a second consumer: its gradient and the bf16 fan-in sum of the two
            ac = 2.0 * (ac + dmid.double().abs())
        a, _ = _merge_abs(ac, gs[0], E["keep_c"], E["kept_c"], None)
        return {"lat_c": a, "lat_f": af}

    return _entry(name, "fpn_chain", make, run, ref, twin, "fine level: d_inner None (`ref = d_inner if d_inner is not None else d_dropped`); "
                  "coarse level: d_inner = the fine level's d_coarse", mid_shape=(B,) + hc + (C,))


# ---- _GroundLogits / _GroundTokenLoss -----------------------------------------------------------------------------------------------
GB, GA, GT = 2, 37, ground_cases.T
LENS = [GT, 37]


def _ground_leaves(name, g, device, log_scale):
    return [("x", AC._bf((GB, GA, GT), g, device)), ("p", AC._bf((GB, GT, GT), g, device, 0.25)),
            ("tbias", AC._randn((GB, GT), g, device) - 2.0), ("log_scale", torch.tensor([log_scale], device=device))]


def _ground_s(L, rn):
    """(clamped logits, raw dot product x inv_scale): the gradient of the raw dot product is what the Functions store as bf16"""
    dt = L["x"].dtype
    dot = rn(torch.matmul(L["x"], L["p"].transpose(1, 2)), fwd=False)
    un = dot * torch.exp(-L["log_scale"].to(dt).reshape(()))
    return (un + L["tbias"].to(dt)[:, None, :]).clamp(-ground_cases.CLAMP, ground_cases.CLAMP), un


def _ground_twin(L, ds_abs):
    """twins of the four inputs from |ds| [B, A, T] (zero where the clamp is active)"""
    x, p = L["x"].double(), L["p"].double()
    inv = torch.exp(-L["log_scale"].double().reshape(()))
    un = torch.matmul(x, p.transpose(1, 2)) * inv
    live = ((un + L["tbias"].double()[:, None, :]).abs() < ground_cases.CLAMP).double()
    ds = ds_abs * live
    return {"x": torch.matmul(ds * inv, p.abs()), "p": torch.matmul((ds * inv).transpose(1, 2), x.abs()), "tbias": ds.sum(1),
            "log_scale": (ds * un.abs()).sum().reshape(1)}


_GROUND_SUMS = {"tbias": "ground_sum", "log_scale": "ground_sum"}


def _logits_entry(name, log_scale, branch):
    def make(device):
        g = AC._gen(name)
        return Case(_ground_leaves(name, g, device, log_scale), ["log_scale"], {}, [AC._randn((GB, GA, GT), g, device)])

    def run(ops, L, E, mid=plain_mid):
        return (mid(ops.ground_logits(L["x"], L["p"], L["tbias"], L["log_scale"]), _ident),)

    def ref(L, E, mid=plain_mid, rn=rn_none):
        return (mid(_ground_s(L, rn)[0], _ident),)

    def twin(L, E, gs, dmid=None):
        return _ground_twin(L, gs[0].double().abs() + (dmid.double().abs() if dmid is not None else 0.0))

    e = _entry(name, "ground", make, run, ref, twin, branch, leaf_family=_GROUND_SUMS, mid_shape=(GB, GA, GT))
    e.clamped = lambda L: (_ground_s({k: v.double() for k, v in L.items()}, rn_none)[1] + L["tbias"].double()[:, None, :]).abs() - ground_cases.CLAMP
    return e


def _loss_entry(name, tdtype, masked, branch):
    alpha, gamma = 0.25, 2.0

    def make(device):
        g = AC._gen(name)
        E = {"targets": ground_cases.targets(GB, GA, LENS, name).to(tdtype).to(device)}
        if masked:
            E["mask"] = ground_cases.text_mask(GB, LENS, name).to(device)
        return Case(_ground_leaves(name, g, device, 0.3), ["log_scale"], E, [torch.tensor(0.75, device=device)])

    def mask_of(E, like):
        return E["mask"] if masked else torch.ones((GB, GT), dtype=torch.uint8, device=like.device)

    def run(ops, L, E, mid=plain_mid):
        return (ops.ground_token_loss(L["x"], L["p"], L["tbias"], L["log_scale"], E["targets"], E.get("mask"), alpha, gamma),)

    def ref(L, E, mid=plain_mid, rn=rn_none):
        s, _ = _ground_s(L, rn)
        return (ground_cases.focal64(s, E["targets"], mask_of(E, s), alpha, gamma).sum().to(s.dtype),)

    def twin(L, E, gs, dmid=None):
        s, _, _ = ground_cases.align64(L["x"], L["p"], L["tbias"], L["log_scale"])
        return _ground_twin(L, (gs[0].double() * ground_cases.focal_grad64(s, E["targets"], mask_of(E, s), alpha, gamma)).abs())

    def zeros(case):
        if not masked:
            return {}
        dead = case.extra["mask"] == 0
        return {"p": dead[:, :, None].expand(GB, GT, GT), "tbias": dead}

    return _entry(name, "ground", make, run, ref, twin, branch, leaf_family=_GROUND_SUMS, zeros=zeros)


# ---- _AtssBoxLosses -----------------------------------------------------------------------------------------------------------------
ATSS_SIZES = [(4, 6), (2, 3), (1, 2)]
ATSS_STRIDES = (8, 16, 32)


def atss_anchors():
    """one square anchor of side 4 stride per location, centred on the cell: [A_l, 4] fp32 per level"""
    out = []
    for (h, w), s in zip(ATSS_SIZES, ATSS_STRIDES):
        cy, cx = torch.meshgrid(torch.arange(h, dtype=torch.float32) * s + s / 2, torch.arange(w, dtype=torch.float32) * s + s / 2, indexing="ij")
        half = 2.0 * s
        out.append(torch.stack([cx - half, cy - half, cx + half - 1, cy + half - 1], -1).reshape(-1, 4))
    return out


# hand-written gts per image (xyxy): about the size of a level-0 / level-1 / level-2 anchor, centred on one
ATSS_TARGETS = {
    "atss-all-levels": [[[5.0, 3.0, 36.0, 33.0], [-12.0, -14.0, 113.0, 110.0]], [[10.0, -8.0, 70.0, 54.0]]],
    "atss-level-empty": [[[5.0, 3.0, 36.0, 33.0]], [[10.0, -8.0, 70.0, 54.0]]],
    "atss-none": [[], []],
}


def _atss_entry(name, branch):
    B = 2
    names = [f"reg{l}" for l in range(3)] + [f"ctr{l}" for l in range(3)]

    def make(device):
        from fiber_amd.modules.grounding_train import pack_targets
        g = AC._gen(name)
        boxes = [torch.tensor(b, dtype=torch.float32).reshape(-1, 4) for b in ATSS_TARGETS[name]]
        n = sum(b.shape[0] for b in boxes)
        pm = torch.zeros((n, atss_cases.T), dtype=torch.uint8)
        pm[torch.arange(n), torch.arange(n) + 1] = 1
        t = pack_targets(boxes, [torch.arange(b.shape[0]) + 1 for b in boxes], pm, gmax=2)
        anchors = atss_anchors()
        a = atss_cases.assign_torch(anchors, t)
        leaves = [(f"reg{l}", AC._randn((B, 4, h, w), g, device) * torch.tensor([3.0, 3.0, 1.5, 1.5], device=device).view(1, 4, 1, 1))
                  for l, (h, w) in enumerate(ATSS_SIZES)]
        leaves += [(f"ctr{l}", 0.5 + 1.5 * AC._randn((B, 1, h, w), g, device)) for l, (h, w) in enumerate(ATSS_SIZES)]
        E = {"anchors": [x.to(device) for x in anchors], "labels": a["labels"].to(device), "reg_targets": a["reg_targets"].to(device),
             "margins": a["margins"], "targets": t.to(device)}
        if torch.device(device).type == "cuda":
            from fiber_amd import ops
            E["assignment"] = ops.atss_assign(E["anchors"], E["targets"], topk=atss_cases.TOPK)
        return Case(leaves, [], E, [torch.tensor(v, device=device) for v in (0.7, 0.3, 1.3)])

    def run_sums(ops, L, E):
        a = E["assignment"]
        return ops._AtssBoxLosses.apply(a.anchors, a.labels, a.reg_targets, list(a.level_off), *[L[k] for k in names])

    def run(ops, L, E, mid=plain_mid):
        return tuple(ops.atss_box_losses([L[f"reg{l}"] for l in range(3)], [L[f"ctr{l}"] for l in range(3)], E["anchors"], E["assignment"]))

    def losses(L, E, gs, dtype):
        g3 = [float(g) if g is not None else 0.0 for g in gs]
        return atss_cases.losses_torch([L[f"reg{l}"] for l in range(3)], [L[f"ctr{l}"] for l in range(3)], E["anchors"], E["labels"],
                                       E["reg_targets"], dtype=dtype, grads=g3)

    def grads(L, E, gs, live, dtype=torch.float64):
        """({leaf: gradient or None}, {leaf: twin}) by atss_cases.losses_torch in `dtype` (fp64: the reference; fp32: the host
        evaluation).  The twin is the ABI bound itself: K_GRAD 2^-23 of atss_cases' gradient magnitudes."""
        r = losses(L, E, gs, dtype)
        G, A, lo = {}, {}, 0
        for l, (h, w) in enumerate(ATSS_SIZES):
            n = h * w
            G[f"reg{l}"], G[f"ctr{l}"] = r["d_bbox_reg"][l], r["d_centerness"][l]
            A[f"reg{l}"] = atss_cases.CONST["K_GRAD"] * atss_cases.EPS * r["grad_mag"][:, lo:lo + n].permute(0, 2, 1).reshape(B, 4, h, w) \
                if "grad_mag" in r else torch.zeros_like(G[f"reg{l}"])
            A[f"ctr{l}"] = atss_cases.CONST["K_GRAD"] * atss_cases.EPS * r["ctr_grad_mag"][:, lo:lo + n].reshape(B, 1, h, w) \
                if "ctr_grad_mag" in r else torch.zeros_like(G[f"ctr{l}"])
            lo += n
        reach = any(g is not None for g in (gs[0], gs[2]))             # sum w does not depend on the predictions
        G = {k: (G[k] if k in live and reach else None) for k in names}
        return G, A, r

    def zeros(case):
        pos = case.extra["labels"] > 0
        out, lo = {}, 0
        for l, (h, w) in enumerate(ATSS_SIZES):
            dead = ~pos[:, lo:lo + h * w].reshape(B, 1, h, w)
            out[f"reg{l}"], out[f"ctr{l}"] = dead.expand(B, 4, h, w), dead
            lo += h * w
        return out

    e = _entry(name, "atss", make, run, None, None, branch, zeros=zeros)
    e.grads, e.run_sums = grads, run_sums
    return e


ENTRIES = [
    _dcn_entry("dcn-c16-s1", 16, 16, "tiled, atomics-free dx (`tiled = need_x and ... C % 16 == 0`); scatter for doffset / dmask with dx = NULL"),
    _dcn_entry("dcn-c16-s2", 16, 16, "as dcn-c16-s1 with stride 2 (8 x 8 tiles)", stride=2),
    _dcn_entry("dcn-c8", 8, 16, "C % 16 != 0: `dxf = torch.zeros(...)`, one scatter launch with fp32 atomics into dxf, `dx = dxf.to(BF16)`", atomics=("x",)),
    _dcn_entry("conv3-c16-bias", 16, 16, "offset = mask = None: no scatter launch (`if dxf is not None or need_off or need_mask`), tiled dx", deform=False),
    _dcn_entry("conv3-c16-nobias", 16, 16, "as conv3-c16-bias with `ctx.has_bias` False: wgrad without the bias sum", deform=False, bias=False),
    _dcn_entry("conv3-c16-27-f32", 16, 27, "Cout = 27: rows padded to Cp = 32 (`if Cp != Cout`), dy fp32 -> bf16 -> pad, dW / db sliced `[:Cout]`; "
               "db alone: `colsum(dy2)[:Cout]`", deform=False, out_fp32=True),
    _dyconv_entry("dyconv"),
    _conv1x1_entry("conv1x1-bias", True), _conv1x1_entry("conv1x1-nobias", False), _conv1x1_entry("conv1x1-nchw", True, nchw=True),
    _fpn_entry("fpn-coarse-keep", (6, 10), (3, 5), True, "both outputs, d_lateral and d_coarse from one launch"),
    _fpn_entry("fpn-coarse-nokeep", (6, 10), (3, 5), False, "`if dropped is None: return inner, None`: keep = NULL in both launches"),
    _fpn_entry("fpn-nocoarse-keep", (6, 10), None, True, "`has_coarse` False: d_coarse = NULL (ScaledDropBlock on a map of its own)"),
    _fpn_entry("fpn-ragged", (7, 9), (4, 5), True, "7 x 9 from 4 x 5: coarse pixels with 1, 2 and 4 children"),
    _fpn_chain_entry("fpn-chain"),
    _logits_entry("logits", 0.3, "`torch.where(out.abs() < 50000.0, ...)` all true; dX on the NT kernel, dP per image on the TN kernel"),
    _logits_entry("logits-clamp", -9.5, "exp(9.5) x the dot products: about a third of the logits beyond +-50000, their ds exactly 0"),
    _loss_entry("loss-u8", torch.uint8, False, "targets uint8 as they are (`targets if targets.dtype == torch.uint8`), text_mask None -> ones"),
    _loss_entry("loss-bool-mask", torch.bool, True, "targets bool -> `(targets != 0).to(torch.uint8)`, dead tokens in the text mask"),
    _loss_entry("loss-u8-mask", torch.uint8, True, "uint8 targets with dead tokens"),
    _atss_entry("atss-all-levels", "positives on all three levels"),
    _atss_entry("atss-level-empty", "no positive on level 2: its launch writes zeros"),
    _atss_entry("atss-none", "num_gt = 0 in both images: all three sums 0 (`if row0:` still folds the zero partials)"),
]
BY_NAME = {e.name: e for e in ENTRIES}
assert len(BY_NAME) == len(ENTRIES) and not set(BY_NAME) & set(AC.BY_NAME)
AUTOGRAD = [e for e in ENTRIES if e.ref is not None]
ATSS = [e for e in ENTRIES if e.family == "atss"]


def reference(entry, case, live, gs, mid=plain_mid, dmid=None):
    """AC.reference for the autograd entries; for the ATSS entries the restatement of atss_cases: ({leaf: gradient or None},
    {leaf: bound}, {leaf: twin})"""
    if entry.ref is not None:
        return AC.reference(entry, case, live, gs, mid, dmid)
    L = leaves_of(case, (), torch.float64)
    G, A, _ = entry.grads(L, case.extra, gs, live)
    return G, {k: AC.bound(entry.fam(k), G[k], A[k]) for k in G if G[k] is not None}, A
