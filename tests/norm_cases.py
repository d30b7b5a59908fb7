"""Case table of the LayerNorm family (csrc/norm.hip, csrc/mlp_rows.hip): every kernel instantiation the default environment reaches,
at a shape that sends the call to it, with the fp64 reference and the per-element bounds.  Shared by tests/test_hip_norm_paths.py
(values against fp64), tests/test_norm_compare_host.py (the bounds on the host) and tools/probes/norm_paths.py (which kernel each
case launched).

LayerNorm (norm.hip): LN_DISPATCH picks (LPR lanes per row, NV 16-byte vectors per lane, U row groups in flight) from nvec = C / 8:
  nvec <= 8: (8, 1, 4)   <= 16: (16, 1, 4)   <= 32: (32, 1, 4)   <= 64: (64, 1, 4)   <= 128: (64, 2, 2 forward / 1 backward)
  <= 256: (64, 4, 1)     <= 384: (64, 6, 1)  <= 512: (64, 8, 1, not PatchMerging)
ln_fwd_kernel<LPR, NV, MERGE, X32, U> / ln_bwd_kernel<...> + ln_bwd_reduce_kernel; X32: the input is the fp32 residual stream.
The forward grid is capped at 4096 workgroups (grid-stride above), the backward at 1024 (fiber_layernorm_bwd_grid); the fold
(ln_bwd_reduce_kernel) adds the backward's one partial row per workgroup in a fixed order: 64 row lanes, each over every 64th row,
then a pairwise tree.
Fused LN-Mlp (mlp_rows.hip): ln_mlp_{fwd,bwd}_kernel<128, 8> and <256, 4>: a wave owns a 32-row strip, a workgroup NW strips.

Reference and bounds: the same formulas in fp64 on the kernels' inputs, bf16 roundings where the kernels perform them, and
  |got - ref| <= base + sum_c CONST[c] * term_c
  STAT  fp32 row statistics (the two-pass mean / variance, rsqrtf), in units of the row's mean |x| (mean) and of 1 (rstd, relative)
  SUM   fp32 row sums of the backward (mean(dy g), mean(dy g xhat)), in units of the matching |.| sums
  RED   dgamma / dbeta: per sequential fp32 add of the kernel's summation (lane over its rows, waves, fold lane, tree), times sum |terms|
  ACC   MFMA fp32 accumulation of the fused kernels' products, in units of |A| |B|
Where the kernel rounds an fp32 intermediate to bf16 (xhat, G = gelu(H), dH of the fused kernels) and the fp64 value lies within the
fp32 error of a rounding boundary, one ulp of that intermediate is allowed and propagated through |W| (abs_mm64); elsewhere the
reference takes the same rounding."""
import math

import torch

from tests.hip_util import abs_mm64, mm64

U = 2.0 ** -8                 # bf16 store: |bf16(v) - v| <= 2^-8 |v|
U32 = 2.0 ** -23              # fp32 store / a few fp32 operations on a stored value
GELU_FWD_ERR = 2.0 ** -20     # common.h gelu2_exact (A&S 7.1.28)
GELU_BWD_ERR = 2.0 ** -12     # common.h gelu_grad2 (clamped minimax polynomial, |err| <= 1.9e-4)
CONST = {"STAT": 2.0 ** -22, "SUM": 2.0 ** -28, "RED": 2.0 ** -30, "ACC": 2.0 ** -25}   # MI355X needed: 2^-22.57, 2^-28.04, 2^-30.12, 2^-25.52
NAN_BF16 = -32768 + 0x7FC0    # bf16 quiet NaN 0xFFC0 as int16
NAN_F32 = -4194304            # fp32 quiet NaN 0xFFC00000 as int32
GUARD = 3                     # guard rows after every row-major output
ROWS = 16384                  # reference row block

LN_UF, LN_UB = 4, 4


def geometry(C, fwd):
    """(LPR, NV, U) of LN_DISPATCH for row width C."""
    nv = C // 8
    if nv <= 64:
        lpr = 8 if nv <= 8 else 16 if nv <= 16 else 32 if nv <= 32 else 64
        return lpr, 1, LN_UF if fwd else LN_UB
    if nv <= 128:
        return 64, 2, 2 if fwd else 1
    return 64, 4 if nv <= 256 else 6 if nv <= 384 else 8, 1


def rows_per_wave(C, fwd=True):
    lpr, _, u = geometry(C, fwd)
    return u * (64 // lpr)


def fwd_grid(rows, C):
    need = -(-rows // (4 * rows_per_wave(C)))
    return min(4096, -(-need // 4))


def bwd_grid(rows):
    return max(1, min(1024, -(-rows // 64)))


def red_depth(rows, C):
    """Sequential fp32 adds behind one dgamma / dbeta element: a lane's rows (U groups per iteration, grid-stride), the RPW rows of
    a wave (shuffle tree), the four waves in turn, the fold lane's partial rows (every 64th), the 64-lane tree."""
    lpr, _, u = geometry(C, False)
    rpw = 64 // lpr
    g = bwd_grid(rows)
    iters = -(-rows // (g * 4 * rpw * u))
    return iters * u + int(math.log2(rpw)) + 3 + -(-g // 64) + 6


def _ln(name, C, rows, x32=False, y32=False, dres=True, eps=1e-5, dist="normal"):
    return dict(kind="ln", name=name, C=C, rows=rows, x32=x32, y32=y32, dres=dres, eps=eps, dist=dist)


def _pm(name, B, H, W, C, x32=False):
    return dict(kind="pm", name=name, B=B, H=H, W=W, C=C, rows=B * (H // 2) * (W // 2), x32=x32, y32=False, dres=False, eps=1e-5,
                dist="normal")


def _mlp(name, C, M, rps=None, g=True):
    return dict(kind="mlp", name=name, C=C, M=M, rps=rps, g=g, eps=1e-5)


# every LN_DISPATCH branch, bf16 forward + backward with the residual gradient; row counts ragged against the row group of a
# workgroup (4 * rows_per_wave), fold lanes with one partial row (below 4033 rows) and with several
CASES = [_ln(f"ln{C}", C, rows) for C, rows in
         ((64, 4133), (96, 517), (128, 4161), (192, 2081), (256, 4097), (384, 1029), (512, 4099), (768, 777), (1024, 4103),
          (1536, 131), (2048, 4105), (3072, 67), (4096, 4107))]
CASES += [
    # the fp32 stream: fp32 input (X32), with and without the residual gradient; bf16 input with an fp32 copy of the output
    _ln("s32-128", 128, 4161, x32=True, dres=False), _ln("s32-512", 512, 2053, x32=True), _ln("s32-768", 768, 4111, x32=True, dres=False),
    _ln("s32-1536", 1536, 515, x32=True), _ln("s32-96", 96, 333, x32=True), _ln("s32-4096", 4096, 70, x32=True, dres=False),
    _ln("y32-384", 384, 1031, y32=True), _ln("y32-768", 768, 4099, y32=True, dres=False), _ln("y32-1024", 1024, 515, y32=True),
    _ln("y32-64", 64, 97, y32=True), _ln("s32-64", 64, 4133, x32=True), _ln("s32-192", 192, 777, x32=True, dres=False),
    _ln("s32-3072", 3072, 133, x32=True),
    # row counts: one row, fewer rows than one row group, past the forward's 4096-workgroup cap at C = 128 (ragged last iteration),
    # past the backward's 1024-workgroup cap (three iterations per wave)
    _ln("rows1", 128, 1, dres=False), _ln("rows13", 64, 13), _ln("rows3-s32", 512, 3, x32=True),
    _ln("fwdcap128", 128, 1048576 + 65 * 17 + 3, dres=False), _ln("bwdcap128-s32", 128, 140001, x32=True),
    # numeric edges: large mean, small spread on the fp32 stream; eps 1e-12
    _ln("bigmean-s32", 512, 2050, x32=True, dist="bigmean"), _ln("bigmean-s32-128", 128, 4163, x32=True, dist="bigmean", dres=False),
    _ln("eps12", 256, 1037, eps=1e-12), _ln("eps12-s32", 768, 301, x32=True, eps=1e-12),
    # PatchMerging at the Swin-B 384^2 merges, a rectangular grid, 4C = 3072 (Swin-L)
    _pm("pm96x96x128", 2, 96, 96, 128), _pm("pm48x48x256", 3, 48, 48, 256), _pm("pm24x24x512", 4, 24, 24, 512),
    _pm("pm14x22x96", 3, 14, 22, 96), _pm("pm12x12x768", 2, 12, 12, 768),
    _pm("pm96x96x128-s32", 2, 96, 96, 128, x32=True), _pm("pm24x24x512-s32", 1, 24, 24, 512, x32=True),
    _pm("pm12x12x768-s32", 3, 12, 12, 768, x32=True), _pm("pm48x48x256-s32", 1, 48, 48, 256, x32=True),
    # the narrow merges no registered model has (4C <= 256), for the templates the dispatcher builds for them
    _pm("pm4x4x16", 5, 4, 4, 16), _pm("pm4x6x16-s32", 3, 4, 6, 16, x32=True), _pm("pm8x8x32", 2, 8, 8, 32),
    _pm("pm8x10x32-s32", 3, 8, 10, 32, x32=True), _pm("pm8x12x64", 3, 8, 12, 64), _pm("pm6x8x64-s32", 2, 6, 8, 64, x32=True),
    # fused LN-Mlp: M ragged against the 32-row strip and the NW * 32-row workgroup (the last workgroup's last waves wholly past M),
    # DropPath rows per sample that are / are not multiples of 32 (a strip in two samples), a dropped sample and 1 / keep scales
    _mlp("mlp128", 128, 808), _mlp("mlp128-nog", 128, 808, g=False), _mlp("mlp128-rs200", 128, 1400, rps=200),
    _mlp("mlp128-rs576", 128, 2304, rps=576), _mlp("mlp128-one", 128, 1, g=True),
    _mlp("mlp256", 256, 420), _mlp("mlp256-rs140", 256, 420, rps=140), _mlp("mlp256-rs88-nog", 256, 1056, rps=88, g=False),
    # the bench's stage 0 at per-GPU batch 32
    _mlp("mlp128-stage0", 128, 32 * 9216, rps=9216),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}


def expected_kernels(case):
    """{"fwd": [templates], "bwd": [templates]} the dispatcher must launch for `case`, as the profiler spells them."""
    tf = lambda v: "true" if v else "false"
    if case["kind"] == "mlp":
        nw = 8 if case["C"] == 128 else 4
        return {"fwd": [f"ln_mlp_fwd_kernel<{case['C']}, {nw}>"], "bwd": [f"ln_mlp_bwd_kernel<{case['C']}, {nw}>"]}
    C = case["C"] if case["kind"] == "ln" else 4 * case["C"]
    merge = case["kind"] == "pm"
    lf, nf, uf = geometry(C, True)
    lb, nb, ub = geometry(C, False)
    return {"fwd": [f"ln_fwd_kernel<{lf}, {nf}, {tf(merge)}, {tf(case['x32'])}, {uf}>"],
            "bwd": [f"ln_bwd_kernel<{lb}, {nb}, {tf(merge)}, {tf(case['x32'])}, {ub}>", "ln_bwd_reduce_kernel"]}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _gen(case, device, seed):
    key = sum(ord(c) * (i + 1) for i, c in enumerate(case["name"]))
    return torch.Generator(device=device).manual_seed(seed + key)


def const_rows(rows):
    """rows set to one constant value (var = 0: xhat = 0, y = beta exactly)"""
    return sorted({0, rows // 2, rows - 1}) if rows >= 8 else []


def make_ln_inputs(case, device="cuda", seed=0):
    """x (bf16, or fp32 for x32 / PatchMerging x32) with columns of unequal scale and a non-zero mean, constant rows, gamma with zeros
    and negative entries, dy and dres (bf16)."""
    g = _gen(case, device, seed)
    if case["kind"] == "pm":
        rows_src, Cs = case["B"] * case["H"] * case["W"], case["C"]
        C = 4 * Cs
    else:
        rows_src, Cs = case["rows"], case["C"]
        C = Cs
    x = (torch.randn(rows_src, Cs, device=device, generator=g) * 1.5 + 0.3) * torch.linspace(0.5, 2.0, Cs, device=device)
    if case["dist"] == "bigmean":
        big = torch.arange(0, rows_src, 5, device=device)
        x[big] = 1000.0 + 1e-2 * torch.randn(len(big), Cs, device=device, generator=g)     # (variance 1e-4 > eps)
    if case["kind"] == "ln":
        for r in const_rows(rows_src):
            x[r] = 0.75
    x = x if case["x32"] else x.to(torch.bfloat16)
    gamma = 1.0 + 0.3 * torch.randn(C, device=device, generator=g)
    gamma[::7] = 0.0
    gamma[3::11] = -0.5 - torch.rand(len(gamma[3::11]), device=device, generator=g)
    beta = 0.2 * torch.randn(C, device=device, generator=g)
    rows = case["rows"]
    dy = torch.randn(rows, C, device=device, generator=g).to(torch.bfloat16)
    inp = dict(x=x, gamma=gamma, beta=beta, dy=dy)
    if case["dres"]:
        inp["dres"] = torch.randn(rows, C, device=device, generator=g).to(torch.bfloat16)
    return inp


def merge_gather(x, B, H, W, C):
    """PatchMerging's concat: row (b, i, j) = x[2i, 2j], x[2i+1, 2j], x[2i, 2j+1], x[2i+1, 2j+1] (4C wide)."""
    v = x.reshape(B, H // 2, 2, W // 2, 2, C)                 # [b, i, di, j, dj, c]; quadrant s = di + 2 dj
    return v.permute(0, 1, 3, 4, 2, 5).reshape(B * (H // 2) * (W // 2), 4 * C)


def merge_scatter(z, B, H, W, C):
    """inverse of merge_gather: [rows, 4C] -> [B * H * W, C]"""
    v = z.reshape(B, H // 2, W // 2, 2, 2, C)                  # [b, i, j, dj, di, c]
    return v.permute(0, 1, 4, 2, 3, 5).reshape(B * H * W, C)


def ln_rows(case, inp):
    """the LayerNorm's input rows [rows, C] (gathered for PatchMerging)"""
    if case["kind"] == "pm":
        return merge_gather(inp["x"], case["B"], case["H"], case["W"], case["C"])
    return inp["x"]


# ---- LayerNorm reference --------------------------------------------------------------------------------------------------------------
def ln_fwd_reference(x, gamma, beta, eps, K=None, dtype=torch.float64):
    """fp64 LayerNorm of rows x ([n, C]) -> (out {y, mean, rstd, xhat}, bounds {name: (base, {const: term})}).
    dtype=torch.float32: the kernel's formula (two-pass statistics) in fp32, for the host tests."""
    K = K or CONST
    x = x.to(dtype)
    C = x.shape[1]
    mu = x.sum(1) / C
    xc = x - mu[:, None]
    var = (xc * xc).sum(1) / C
    rstd = torch.rsqrt(var + eps)
    xhat = xc * rstd[:, None]
    g, b = gamma.to(dtype), beta.to(dtype)
    y = xhat * g + b
    out = dict(y=y, mean=mu, rstd=rstd, xhat=xhat)
    if dtype != torch.float64:
        return out, None
    S = x.abs().mean(1)
    e_mu = K["STAT"] * S
    # |xhat| error in units of STAT: the mean's error (STAT S) through rstd, rstd's relative error (STAT) times |xhat|; the mean's
    # error also enters the variance squared (quad)
    e_xh = (rstd * S)[:, None] + xhat.abs()
    quad = xhat.abs() * ((e_mu * rstd) ** 2)[:, None]
    ga = g.abs()
    st32 = U32 * (xhat.abs() * ga + b.abs())
    bounds = {
        "y": (U * y.abs() + ga * quad + st32, {"STAT": ga * e_xh}),
        "y32": (ga * quad + st32, {"STAT": ga * e_xh}),
        "mean": (torch.zeros_like(mu), {"STAT": S}),
        "rstd": (rstd * (e_mu * rstd) ** 2, {"STAT": rstd}),
    }
    return out, bounds


def ln_bwd_reference(x, dy, gamma, mean, rstd, dres, case, K=None, dtype=torch.float64):
    """fp64 LayerNorm backward from the SAVED statistics (mean, rstd as the kernel reads them) -> (out {dx, dgamma, dbeta}, bounds).
    x: [n, C] rows (gathered for PatchMerging)."""
    K = K or CONST
    x, dy, g = x.to(dtype), dy.to(dtype), gamma.to(dtype)
    mean, rstd = mean.to(dtype), rstd.to(dtype)
    C = x.shape[1]
    xhat = (x - mean[:, None]) * rstd[:, None]
    dg = dy * g
    s1 = dg.sum(1, keepdim=True) / C
    s2 = (dg * xhat).sum(1, keepdim=True) / C
    br = rstd[:, None] * (dg - s1 - xhat * s2)
    dx = br + dres.to(dtype) if dres is not None else br
    dgamma, dbeta = (dy * xhat).sum(0), dy.sum(0)
    out = dict(dx=dx, dgamma=dgamma, dbeta=dbeta)
    if dtype != torch.float64:
        return out, None
    adg = dg.abs()
    sum_term = rstd[:, None] * (adg + adg.mean(1, keepdim=True) + xhat.abs() * (adg * xhat.abs()).mean(1, keepdim=True))
    # xhat in fp32: (x - mean) and * rstd each round once; dy * g once
    ops_term = 4 * U32 * rstd[:, None] * (adg + xhat.abs() * (adg * xhat.abs()).mean(1, keepdim=True)) + U32 * dx.abs()
    n = red_depth(x.shape[0], C)
    bounds = {
        "dx": (U * dx.abs() + ops_term, {"SUM": sum_term}),
        "dgamma": (4 * U32 * (dy * xhat).abs().sum(0), {"RED": n * (dy * xhat).abs().sum(0)}),
        "dbeta": (torch.zeros_like(dbeta), {"RED": n * dy.abs().sum(0)}),
    }
    return out, bounds


# ---- fused LN-Mlp ---------------------------------------------------------------------------------------------------------------------
def fa_perm(K, device):
    """the kernels' hidden order: position p holds logical index p with bits 2 and 3 swapped (ops._fa)"""
    i = torch.arange(K, device=device)
    return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1)


def make_mlp_inputs(case, device="cuda", seed=0):
    """x, dy (bf16 [M, C]); w1p = W1 diag(gamma) (bf16 [4C, C]), b1p (fp32, a distinct value per hidden unit), w2 (bf16 [C, 4C],
    logical order), b2; rowscale: sample 1 dropped, the others 1 / keep = 1.25 or their own factor."""
    g = _gen(case, device, seed)
    C, M = case["C"], case["M"]
    H = 4 * C
    x = ((torch.randn(M, C, device=device, generator=g) * 1.3 + 0.2) * torch.linspace(0.6, 1.6, C, device=device)).to(torch.bfloat16)
    x[M // 3] = 0.5                                            # one constant row
    w1p = (torch.randn(H, C, device=device, generator=g) * C ** -0.5 * torch.linspace(1.4, 0.6, H, device=device)[:, None]).to(torch.bfloat16)
    b1p = 0.25 * torch.randn(H, device=device, generator=g) + torch.linspace(-0.5, 0.5, H, device=device)
    w2 = (torch.randn(C, H, device=device, generator=g) * H ** -0.5).to(torch.bfloat16)
    b2 = 0.1 * torch.randn(C, device=device, generator=g)
    inp = dict(x=x, w1p=w1p, b1p=b1p, w2=w2, b2=b2, dy=torch.randn(M, C, device=device, generator=g).to(torch.bfloat16))
    if case["rps"]:
        ns = M // case["rps"]
        rs = torch.full((ns,), 1.25, device=device)
        rs[2::3] = 0.75 + 0.125 * torch.arange(len(rs[2::3]), device=device)
        if ns > 1:
            rs[1] = 0.0
        inp["rowscale"] = rs
    p = fa_perm(H, device)
    inp["w2p"] = inp["w2"][:, p].contiguous()                 # FA(W2) [C, 4C]
    inp["w2tp"] = inp["w2"].t().contiguous()                  # W2^T [4C, C]
    inp["w1tp"] = inp["w1p"].t()[:, p].contiguous()           # FA(W1'^T) [C, 4C]
    return inp


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.5 ** 0.5))


def dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x * 0.5 ** 0.5)) + x * torch.exp(-0.5 * x * x) * (2 * math.pi) ** -0.5


def bf16r(v):
    return v.to(torch.float32).to(torch.bfloat16).to(v.dtype)


def straddle(v, e):
    """width of the bf16 rounding interval v +- e straddles (0 where bf16(v - e) == bf16(v + e): the kernel rounds as the reference)"""
    return (bf16r(v + e) - bf16r(v - e)).abs()


def row_scale(case, inp, i, j, device):
    if "rowscale" not in inp:
        return torch.ones(j - i, 1, dtype=torch.float64, device=device)
    m = torch.arange(i, j, device=device)
    return inp["rowscale"].double()[m // case["rps"]][:, None]


def mlp_reference(case, inp, i, j, K=None, want_bwd=True, hid_order=None):
    """Rows [i, j) of the fused LN-Mlp in fp64 with the kernels' bf16 roundings (xhat, G, dH) -> (out, bounds).
    hid_order (host tests): a permutation of the hidden index applied to W2's columns in the forward (a wrong K order)."""
    K = K or CONST
    x = inp["x"][i:j].double()
    C = x.shape[1]
    w1p, w2 = inp["w1p"].double(), inp["w2"].double()
    if hid_order is not None:
        w2 = w2[:, hid_order]
    b1p, b2 = inp["b1p"].double(), inp["b2"].double()
    s = row_scale(case, inp, i, j, x.device)
    st, sb = ln_fwd_reference(x, torch.ones(C, dtype=torch.float64, device=x.device), torch.zeros(C, dtype=torch.float64, device=x.device),
                              case["eps"], K)
    xhat, rstd = st["xhat"], st["rstd"]
    e_xh = K["STAT"] * sb["y"][1]["STAT"] + sb["y"][0] - U * st["y"].abs() - U32 * xhat.abs()   # |xhat| error of the fp32 statistics
    xr = bf16r(xhat)
    a_xh = straddle(xhat, e_xh)
    ab1 = abs_mm64(xr, w1p) + b1p.abs()
    Hm = mm64(xr, w1p) + b1p
    errH = K["ACC"] * ab1 + abs_mm64(a_xh, w1p)
    G = gelu64(Hm)
    eG = (dgelu64(Hm).abs() + 0.8 * errH) * errH + GELU_FWD_ERR
    Gr = bf16r(G)
    a_G = straddle(G, eG)
    Y = mm64(Gr, w2) + b2
    y = x + s * Y
    out = dict(y=y, g=G, xhat=xhat)
    bounds = {"y": (U * y.abs() + s * abs_mm64(a_G, w2) + 2 * U32 * (x.abs() + s * Y.abs()), {"ACC": s * abs_mm64(Gr, w2)}),
              "g": (U * G.abs() + (dgelu64(Hm).abs() + 0.8 * errH) * abs_mm64(a_xh, w1p) + GELU_FWD_ERR,
                    {"ACC": (dgelu64(Hm).abs() + 0.8 * errH) * ab1}),
              "xhat": (sb["y"][0] - U32 * xhat.abs(), {"STAT": sb["y"][1]["STAT"]})}
    if not want_bwd:
        return out, bounds
    dy = inp["dy"][i:j].double()
    w2t = w2.t()
    dG = mm64(dy, w2t)                                        # dy W2: [rows, 4C]
    adG = abs_mm64(dy, w2t)
    gp = dgelu64(Hm)
    dH = s * dG * gp
    e_dH_acc = s * (gp.abs() * adG + dG.abs() * 0.8 * ab1)
    e_dH_base = s * dG.abs() * (GELU_BWD_ERR + 0.8 * abs_mm64(a_xh, w1p))
    dHr = bf16r(dH)
    a_dH = straddle(dH, e_dH_base + K["ACC"] * e_dH_acc)
    w1pt = w1p.t()
    a = mm64(dHr, w1pt)                                       # dxhat = dH W1': [rows, C]
    ea_acc = abs_mm64(dHr, w1pt)
    ea_base = abs_mm64(a_dH, w1pt)
    s1 = a.mean(1, keepdim=True)
    s2 = (a * xr).mean(1, keepdim=True)
    r = rstd[:, None]
    dx = dy + r * (a - s1 - xr * s2)
    axr = xr.abs()
    prop = lambda e: r * (e + e.mean(1, keepdim=True) + axr * (e * axr).mean(1, keepdim=True))
    base_dx = (U * dx.abs() + prop(ea_base) + r * (a_xh * s2.abs() + axr * (a.abs() * a_xh).mean(1, keepdim=True))
               + 4 * U32 * r * (a.abs() + axr * (a * xr).abs().mean(1, keepdim=True)))
    sum_dx = r * (a.abs() + a.abs().mean(1, keepdim=True) + axr * (a * xr).abs().mean(1, keepdim=True))
    # rstd's own fp32 error (relative STAT) times the LayerNorm branch
    stat_dx = r * (a - s1 - xr * s2).abs()
    out.update(dx=dx, dh=dH)
    bounds.update(dx=(base_dx, {"ACC": prop(ea_acc), "SUM": sum_dx, "STAT": stat_dx}),
                  dh=(U * dH.abs() + e_dH_base, {"ACC": e_dH_acc}))
    return out, bounds


# ---- runners (C ABI, every output NaN-filled with GUARD rows / elements after it) -----------------------------------------------------
def nan_buf(shape, dtype, device="cuda"):
    t = torch.empty(shape, dtype=dtype, device=device)
    (t.view(torch.int16) if dtype == torch.bfloat16 else t.view(torch.int32)).fill_(NAN_BF16 if dtype == torch.bfloat16 else NAN_F32)
    return t


def ln_width(case):
    return case["C"] if case["kind"] == "ln" else 4 * case["C"]


def run_ln_fwd(lib, case, inp):
    """-> {"y", "y32", "mean", "rstd"}: buffers with GUARD rows (the case's rows first)"""
    rows, C, dev = case["rows"], ln_width(case), inp["x"].device
    o = dict(y=nan_buf((rows + GUARD, C), torch.bfloat16, dev), mean=nan_buf(rows + GUARD, torch.float32, dev),
             rstd=nan_buf(rows + GUARD, torch.float32, dev))
    if case["y32"]:
        o["y32"] = nan_buf((rows + GUARD, C), torch.float32, dev)
    P = lib.ptr
    x, g, b = inp["x"], inp["gamma"], inp["beta"]
    if case["kind"] == "pm":
        dims = (case["B"], case["H"], case["W"], case["C"], case["eps"])
        if case["x32"]:
            lib.call("fiber_patch_merge_ln_fwd_stream", P(x), P(g), P(b), P(o["y"]), P(o["mean"]), P(o["rstd"]), *dims, 1)
        else:
            lib.call("fiber_patch_merge_ln_fwd_bf16", P(x), P(g), P(b), P(o["y"]), P(o["mean"]), P(o["rstd"]), *dims)
    elif not case["x32"] and not case["y32"]:
        lib.call("fiber_layernorm_fwd_bf16", P(x), P(g), P(b), P(o["y"]), P(o["mean"]), P(o["rstd"]), rows, C, case["eps"])
    else:
        lib.call("fiber_layernorm_fwd_stream", P(x), P(g), P(b), P(o["y"]), P(o.get("y32")), P(o["mean"]), P(o["rstd"]), rows, C,
                 case["eps"], 1 if case["x32"] else 0)
    return o


def run_ln_bwd(lib, case, inp, fwd):
    """-> {"dx", "dgamma", "dbeta", "ws"}: buffers with GUARD rows / elements after them (dx of PatchMerging: the source tensor)"""
    rows, C, dev = case["rows"], ln_width(case), inp["x"].device
    nsrc = inp["x"].shape[0]
    ws_n = lib.plain("fiber_layernorm_bwd_grid", rows) * 8 * C
    o = dict(dx=nan_buf((nsrc + GUARD, inp["x"].shape[1]), torch.bfloat16, dev), dgamma=nan_buf(C + GUARD, torch.float32, dev),
             dbeta=nan_buf(C + GUARD, torch.float32, dev), ws=nan_buf(ws_n + 64, torch.float32, dev))
    P = lib.ptr
    args = (P(inp["dy"]), P(inp["x"]), P(inp["gamma"]), P(fwd["mean"]), P(fwd["rstd"]))
    outs = (P(o["dx"]), P(o["dgamma"]), P(o["dbeta"]), P(o["ws"]))
    if case["kind"] == "pm":
        dims = (case["B"], case["H"], case["W"], case["C"])
        if case["x32"]:
            lib.call("fiber_patch_merge_ln_bwd_stream", *args, *outs, *dims, 1)
        else:
            lib.call("fiber_patch_merge_ln_bwd_bf16", *args, *outs, *dims)
    elif case["x32"] or case["y32"]:
        lib.call("fiber_layernorm_bwd_stream", *args, P(inp.get("dres")), *outs, rows, C, 1 if case["x32"] else 0)
    else:
        lib.call("fiber_layernorm_bwd_bf16", *args, P(inp.get("dres")), *outs, rows, C)
    return o


def run_mlp_fwd(lib, case, inp, with_g=None):
    M, C, dev = case["M"], case["C"], inp["x"].device
    with_g = case["g"] if with_g is None else with_g
    o = dict(y=nan_buf((M + GUARD, C), torch.bfloat16, dev))
    if with_g:
        o["g"] = nan_buf((M + GUARD, 4 * C), torch.bfloat16, dev)
    P = lib.ptr
    lib.call("fiber_ln_mlp_fwd_bf16", P(inp["x"]), P(inp["w1p"]), P(inp["b1p"]), P(inp["w2p"]), P(inp["b2"]), P(inp.get("rowscale")),
             P(o["y"]), P(o.get("g")), M, C, case["rps"] or 0, case["eps"])
    return o


def run_mlp_bwd(lib, case, inp):
    M, C, dev = case["M"], case["C"], inp["x"].device
    o = dict(dx=nan_buf((M + GUARD, C), torch.bfloat16, dev), dh=nan_buf((M + GUARD, 4 * C), torch.bfloat16, dev),
             xhat=nan_buf((M + GUARD, C), torch.bfloat16, dev))
    P = lib.ptr
    lib.call("fiber_ln_mlp_bwd_bf16", P(inp["x"]), P(inp["dy"]), P(inp["w1p"]), P(inp["b1p"]), P(inp["w2tp"]), P(inp["w1tp"]),
             P(inp.get("rowscale")), P(o["dx"]), P(o["dh"]), P(o["xhat"]), M, C, case["rps"] or 0, case["eps"])
    return o
