"""Case table of the deformable-convolution sampling kernels (csrc/dcn.hip): every kernel and instantiation, at the smallest shape that
reaches it, with the fp64 reference and the per-element bounds.  Shared by tests/test_hip_dcn_paths.py (values against fp64),
tests/test_dcn_optim_compare_host.py (the reference against oracle/dcn_ref.py, the bounds against mutations) and
tools/probes/dcn_optim_paths.py (which kernel each case launched).  Nothing here needs a GPU to import; the runners at the end do.

The operation, channels-last and tap-major (x [B, H, W, C], offset [M, 2 T] as (dy, dx) per tap, mask [M, T], cols / dcols [M, T C],
M = B Ho Wo, T = kh kw, tap t = i kw + j):
  h = float32(ho stride - pad + i) + offset[m, 2t]        ONE fp32 addition: the ABI's definition of the sampling coordinate
  w = float32(wo stride - pad + j) + offset[m, 2t + 1]
  taken when -1 < h < H and -1 < w < W; h0 = floor(h), lh = h - h0 (likewise w); corner (h0 + a, w0 + b) counts when it lies in the map
  cols[m, t, c]   = mask[m, t] sum_ab wt_ab x[b, h0 + a, w0 + b, c]                 wt = ((1 - lh) | lh) ((1 - lw) | lw)
  dx[b, y, x, c] += wt_ab mask[m, t] dcols[m, t, c]                                   for every (m, t, a, b) whose corner is (y, x)
  dmask[m, t]     = sum_c dcols[m, t, c] sum_ab wt_ab x[...]
  doffset[m, 2t]  = mask[m, t] sum_c dcols[m, t, c] ((1 - lw) (x10 - x00) + lw (x11 - x01))      (the right derivative on integers)
The coordinate is formed with numpy.float32 and everything after it in fp64: floor, the `in` test and the four corner flags then agree
with the kernels exactly, so every element of every output is compared.

Bounds, |got - ref| <= base + sum_c CONST[c] 2^-24 term_c:
  bf16 store    half an ulp of bf16 at ref: 2^-9 times the power of two above |ref| (2^-9 |ref| itself is below half an ulp unless
                ref is a power of two, so no correctly rounded store could meet it), at least 2^-134 (bf16 denormals)
  CORNER        the gather's fp32 4-corner sum, term = mask sum_ab |wt_ab x_ab|
  CH            dmask / doffset: the fp32 channel sum of a lane, its shuffle tree, term = sum_c |dcol| sum |wt x| (and the derivative's form)
  DX            dx: the fp32 corner weight, its product with dcol and the fp32 atomic adds that meet at a pixel, term = sum |wt mask dcol|
  tiled dx      n(y, x) 2^(e - 20), exact: n = contributions accumulated in a window for that pixel, 2^e the power of two above max |dcols|;
                each is rounded to nearest at 2^(e - 19).  The fp32 weight product in front of that rounding and the `far` atomics are a DX chain.
Each constant has a ceiling (ceilings()): twice the number of fp32 operations on the chain's longest path for the case's C and G."""
import math

import numpy as np
import torch

BF16_STORE = 2.0 ** -9
BF16_TINY = 2.0 ** -134


def bf16_store(ref):
    """half an ulp of bf16 at ref: BF16_STORE times the power of two above |ref| (ref = f 2^e, 0.5 <= f < 1: 2^(e - 9)), 0 at 0, and
    never below half the spacing of the bf16 denormals"""
    e = np.frexp(np.abs(ref))[1].astype(np.float64)
    return np.where(ref == 0, 0.0, np.maximum(BF16_STORE * np.exp2(e), BF16_TINY))

F32 = 2.0 ** -24
CONST = {"CORNER": 8.0, "CH": 8.0, "DX": 8.0}   # MI355X needed: see profiles/dcn_optim_pins.md
NAN_BF16 = -32768 + 0x7FC0    # bf16 quiet NaN 0xFFC0 as int16
NAN_F32 = -4194304            # fp32 quiet NaN 0xFFC00000 as int32 (also the fill of the fixed-point windows)
GUARD = 64                    # guard elements after every output
WIN, HALO = 24, 3             # dcn.hip DCN_WIN, DCN_HALO
SCATTER_C = (8, 16, 24, 32, 64, 128, 256, 512, 520)


def scatter_group(C):
    """G of the dcn_scatter_kernel<G> that fiber_dcn_scatter_bf16 launches: the largest power of two <= min(C / 8, 64)"""
    return min(64, 1 << int(math.log2(C // 8)))


def _case(name, kind, B, H, W, C, stride, off="mix", mask=True, dcols="randn", **kw):
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    return dict(name=name, kind=kind, B=B, H=H, W=W, C=C, stride=stride, pad=1, kh=3, kw=3, Ho=Ho, Wo=Wo, M=B * Ho * Wo, T=9,
                off=off, mask=mask, dcols=dcols, **kw)


GATHER_CASES = [
    _case("g_c8", "gather", 1, 5, 6, 8, 1),
    _case("g_c24_s2", "gather", 2, 7, 9, 24, 2),
    _case("g_c520", "gather", 1, 5, 6, 520, 1),
    _case("g_c64_rand", "gather", 2, 13, 17, 64, 1, off="randn"),
    _case("g_plain_s1", "gather", 1, 5, 6, 16, 1, off=None, mask=False),
    _case("g_plain_s2", "gather", 2, 7, 9, 16, 2, off=None, mask=False),
    _case("g_offset_only", "gather", 1, 5, 6, 8, 1, mask=False),
    _case("g_mask_only", "gather", 1, 5, 6, 8, 1, off=None),
    _case("g_all_outside", "gather", 1, 5, 6, 16, 1, off="outside"),
]
SCATTER_CASES = [_case(f"s_c{C}_s1", "scatter", 1, 5, 6, C, 1) for C in SCATTER_C] + \
                [_case(f"s_c{C}_s2", "scatter", 2, 7, 9, C, 2) for C in SCATTER_C] + \
                [_case("s_c64_rand", "scatter", 2, 13, 17, 64, 1, off="randn"), _case("s_plain", "scatter", 1, 5, 6, 16, 1, off=None, mask=False)]
TILED_CASES = [
    _case("t_one", "tiled", 1, 16, 16, 16, 1),
    _case("t_seams", "tiled", 2, 33, 33, 32, 1),
    _case("t_s2", "tiled", 1, 19, 35, 48, 2),
    _case("t_rand", "tiled", 1, 19, 35, 16, 1, off="randn"),
    _case("t_far", "tiled", 1, 33, 33, 16, 1, off="far"),
    _case("t_plain", "tiled", 1, 33, 33, 16, 1, off=None, mask=False),
    _case("t_zero", "tiled", 1, 16, 16, 16, 1, dcols="zero"),
    _case("t_max_1", "tiled", 1, 16, 16, 16, 1, dcols=1.0),
    _case("t_max_below_1", "tiled", 1, 16, 16, 16, 1, dcols=0.99609375),
    _case("t_max_2p120", "tiled", 1, 16, 16, 16, 1, dcols=2.0 ** 120),
    _case("t_max_denormal", "tiled", 1, 16, 16, 16, 1, dcols=100 * 2.0 ** -133),
    _case("t_pile", "tiled", 1, 16, 16, 16, 1, off=("pile", 8, 8), mask="ones", dcols="pile"),
    # the same pile-up under FOUR windows (pixel (16, 16) of a 32 x 32 map lies in all of them): 4 x 2304 full-size contributions, more
    # than one int32 holds once the windows are added
    _case("t_pile4", "tiled", 1, 32, 32, 16, 1, off=("pile", 16, 16), mask="ones", dcols="pile"),
]
CASES = GATHER_CASES + SCATTER_CASES + TILED_CASES
CASE_BY_NAME = {c["name"]: c for c in CASES}
PILE_VALUE = 1.9921875


def expected_kernels(case):
    if case["kind"] == "gather":
        return ["dcn_gather_kernel"]
    if case["kind"] == "scatter":
        return [f"dcn_scatter_kernel<{scatter_group(case['C'])}>"]
    return ["absmax_bf16_kernel", "dcn_dx_sum_kernel", "dcn_dx_tile_kernel"]


def tiling(case):
    T = 16 if case["stride"] == 1 else 8
    return T, -(-case["Ho"] // T), -(-case["Wo"] // T)


def workspace_words(case):
    """fiber_dcn_dx_workspace's formula: the windows, the `far` map, the scale word (+ 3 of padding)"""
    _, ty, tx = tiling(case)
    return case["B"] * ty * tx * WIN * WIN * case["C"] + case["B"] * case["H"] * case["W"] * case["C"] + 4


def ceilings(case, n_max=0):
    """twice the fp32 operations on the longest path.  CORNER: lh, 1 - lh, the weight product, * mask, * x, three adds.  CH: the same
    inner sum without the mask, * dcol, the lane's 8 ceil(C8 / G) adds, log2 G shuffle adds, * mask.  DX: lh, 1 - lh, weight product,
    * mask, * dcol and the n_max adds that meet at the busiest pixel."""
    C8, G = case["C"] // 8, scatter_group(case["C"])
    return {"CORNER": 2.0 * 8, "CH": 2.0 * (9 + 8 * -(-C8 // G) + int(math.log2(G))), "DX": 2.0 * (5 + max(n_max, 1))}


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def _bf16_exact(t):
    return t.to(torch.bfloat16).double().numpy()


def base_coords(case):
    """integer tap positions (ho stride - pad + i, wo stride - pad + j) as [M, T] arrays, and the image index [M]"""
    m = np.arange(case["M"])
    wo, ho, b = m % case["Wo"], (m // case["Wo"]) % case["Ho"], m // (case["Wo"] * case["Ho"])
    t = np.arange(case["T"])
    bh = ho[:, None] * case["stride"] - case["pad"] + t[None] // case["kw"]
    bw = wo[:, None] * case["stride"] - case["pad"] + t[None] % case["kw"]
    return bh, bw, b


def _mix_axis(base, n, idx, period, lat):
    """one coordinate axis of the mixed offsets: lattice offsets, and by (sample index % period): an exact integer coordinate, exactly -1
    and exactly n (not taken), inside (-1, 0) and (n - 1, n) (two corners), exactly n - 1 (l = 0, the upper corner invalid)"""
    off = lat.copy()
    k = idx % period
    off[k == 0] = np.round(lat[k == 0])
    for sel, coord in ((1, -1.0), (2, float(n)), (3, -0.28125), (4, n - 1 + 0.640625), (5, float(n - 1))):
        off[k == sel] = coord - base[k == sel]
    return off


def make_offsets(case, seed=0):
    """fp32 [M, 2 T] or None.  "mix": every value on the 1/64 lattice (the fp32 addition is exact); "randn": sigma = 1.2 px, any fp32;
    "far": up to +-7 px but the sample kept inside the map, some placed half a pixel across their window's last row / column;
    "outside": +-1e4; ("pile", y, x): integer offsets steering every sample onto pixel (y, x)."""
    kind = case["off"]
    if kind is None:
        return None
    g = torch.Generator().manual_seed(1000 + seed)
    M, T, H, W = case["M"], case["T"], case["H"], case["W"]
    bh, bw, _ = base_coords(case)
    idx = np.arange(M * T).reshape(M, T)
    if kind == "randn":
        o = (torch.randn(M, 2 * T, generator=g) * 1.2).numpy().astype(np.float32)
        return o
    lat = lambda r: (torch.randint(-r * 64, r * 64 + 1, (M, T), generator=g).double() / 64).numpy()
    if kind == "mix":
        oh, ow = _mix_axis(bh, H, idx, 8, lat(2)), _mix_axis(bw, W, idx // 8 + idx, 7, lat(2))
    elif kind == "far":
        h, w = np.clip(bh + lat(7), 0, H - 1), np.clip(bw + lat(7), 0, W - 1)
        edge = -case["pad"] - HALO + WIN - 1                                        # last row / column of the first window: 19
        m = np.arange(M)
        ho, wo = (m // case["Wo"]) % case["Ho"], m % case["Wo"]
        h[(ho >= 14) & (ho < 16), 0] = edge + 0.5                                     # tile row 0: corner row 19 in LDS, row 20 in `far`
        w[(wo >= 14) & (wo < 16), 1] = edge + 0.5
        oh, ow = h - bh, w - bw
    elif kind == "outside":
        sign = np.where(idx % 2 == 0, 1.0, -1.0)
        oh, ow = 1e4 * sign, -1e4 * sign * np.where(idx % 3 == 0, 1.0, -1.0)
    else:
        oh, ow = kind[1] - bh.astype(np.float64), kind[2] - bw.astype(np.float64)
    o = np.empty((M, 2 * T), np.float32)
    o[:, 0::2], o[:, 1::2] = oh, ow
    return o


def make_inputs(case, seed=0):
    """numpy: x [B, H, W, C] and dcols [M, T C] float64 holding bf16-exact values, offset / mask float32 or None"""
    g = torch.Generator().manual_seed(seed)
    B, H, W, C, M, T = (case[k] for k in ("B", "H", "W", "C", "M", "T"))
    x = _bf16_exact(torch.randn(B, H, W, C, generator=g) * 1.5 + 0.25)
    mask = None
    if case["mask"] == "ones":
        mask = np.ones((M, T), np.float32)
    elif case["mask"]:
        mask = torch.sigmoid(torch.randn(M, T, generator=g) * 2).clamp_min(2.0 ** -20).numpy().astype(np.float32)
        mask[::5, 0] = 1.0
    d = case["dcols"]
    if d == "zero":
        dcols = np.zeros((M, T * C))
    elif d == "pile":
        dcols = np.full((M, T * C), PILE_VALUE)
    else:
        dcols = _bf16_exact(torch.randn(M, T * C, generator=g))
        if d != "randn":                                       # the largest magnitude exactly d, once, with a negative sign
            dcols = _bf16_exact(torch.from_numpy(dcols / (np.abs(dcols).max() * 1.01) * d))
            assert np.abs(dcols).max() < d
            dcols[M // 2, 5] = -d
    return dict(x=x, offset=make_offsets(case, seed), mask=mask, dcols=dcols)


# ---- the fp64 reference ------------------------------------------------------------------------------------------------------------------
def sample_geometry(case, offset, mutate=None):
    """The (position, tap) geometry from the fp32 coordinate.  mutate: "border" takes the right-border rule as w0 + 1 <= W,
    "left" moves samples on an integer coordinate to the cell on their left (the same sample, the left derivative)."""
    H, W = case["H"], case["W"]
    bh, bw, b = base_coords(case)
    h, w = bh.astype(np.float32), bw.astype(np.float32)
    if offset is not None:
        assert offset.dtype == np.float32
        h, w = h + offset[:, 0::2], w + offset[:, 1::2]           # float32 + float32: the one fp32 addition
    inn = (h > np.float32(-1)) & (w > np.float32(-1)) & (h < np.float32(H)) & (w < np.float32(W))
    fh, fw = np.floor(h), np.floor(w)
    h0, w0 = fh.astype(np.int64), fw.astype(np.int64)
    lh, lw = h.astype(np.float64) - fh.astype(np.float64), w.astype(np.float64) - fw.astype(np.float64)
    if mutate == "left":
        sh, sw = inn & (lh == 0), inn & (lw == 0)
        h0, lh = np.where(sh, h0 - 1, h0), np.where(sh, 1.0, lh)
        w0, lw = np.where(sw, w0 - 1, w0), np.where(sw, 1.0, lw)
    wmax = W if mutate == "border" else W - 1
    ok = [inn & (h0 >= 0) & (w0 >= 0), inn & (h0 >= 0) & (w0 + 1 <= wmax),
          inn & (h0 + 1 <= H - 1) & (w0 >= 0), inn & (h0 + 1 <= H - 1) & (w0 + 1 <= wmax)]
    wt = [(1 - lh) * (1 - lw), (1 - lh) * lw, lh * (1 - lw), lh * lw]
    return dict(b=b, h0=h0, w0=w0, lh=lh, lw=lw, inn=inn, ok=ok, wt=wt)


def reference(case, inp, grads=True, mutate=None, windows=False):
    """fp64 results and bound terms.  cols, cols_abs [M, T C]; with grads: dx, dx_abs, dx_n [B, H, W, C] / [B, H, W], dmask, dmask_abs [M, T],
    doffset, doffset_abs [M, 2 T]; for the tiled kernels the split of dx: dx_far, far_abs, n_win, n_far (contributions whose corner
    leaves the window of their tile), straddle (samples with corners on both sides) and, with windows=True, win [tiles, 24, 24, C]."""
    B, H, W, C, M, T = (case[k] for k in ("B", "H", "W", "C", "M", "T"))
    g = sample_geometry(case, inp["offset"], mutate)
    mk = np.ones((M, T)) if inp["mask"] is None else inp["mask"].astype(np.float64)
    xf = inp["x"].reshape(B * H * W, C)
    flat, vals = [], []
    for k, (a, bb) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        idx = (g["b"][:, None] * H + g["h0"] + a) * W + g["w0"] + bb              # memory-linear, as the kernels index
        idx = np.clip(np.where(g["ok"][k], idx, 0), 0, B * H * W - 1)
        flat.append(idx)
        vals.append(xf[idx] * g["ok"][k][..., None])
    samp = sum(g["wt"][k][..., None] * vals[k] for k in range(4))
    samp_abs = sum(g["wt"][k][..., None] * np.abs(vals[k]) for k in range(4))
    out = dict(cols=(samp * mk[..., None]).reshape(M, T * C), cols_abs=(samp_abs * mk[..., None]).reshape(M, T * C), geom=g)
    if not grads:
        return out
    G = inp["dcols"].reshape(M, T, C)
    Ga = np.abs(G)
    out["e"] = fixed_exponent(inp["dcols"])
    out["dmask"], out["dmask_abs"] = (G * samp).sum(-1), (Ga * samp_abs).sum(-1)
    v00, v01, v10, v11 = vals
    hh, hw, lh, lw = (1 - g["lh"])[..., None], (1 - g["lw"])[..., None], g["lh"][..., None], g["lw"][..., None]
    gh, gw = hw * (v10 - v00) + lw * (v11 - v01), hh * (v01 - v00) + lh * (v11 - v10)
    gha = hw * (np.abs(v10) + np.abs(v00)) + lw * (np.abs(v11) + np.abs(v01))
    gwa = hh * (np.abs(v01) + np.abs(v00)) + lh * (np.abs(v11) + np.abs(v10))
    doff, doffa = np.empty((M, 2 * T)), np.empty((M, 2 * T))
    doff[:, 0::2], doff[:, 1::2] = mk * (G * gh).sum(-1), mk * (G * gw).sum(-1)
    doffa[:, 0::2], doffa[:, 1::2] = mk * (Ga * gha).sum(-1), mk * (Ga * gwa).sum(-1)
    out["doffset"], out["doffset_abs"] = doff, doffa
    # dx, and its split by the tile windows of dcn_dx_tile_kernel
    Tt, tiles_y, tiles_x = tiling(case)
    m = np.arange(M)
    ty, tx = ((m // case["Wo"]) % case["Ho"]) // Tt, (m % case["Wo"]) // Tt
    y0, x0 = ty * Tt * case["stride"] - case["pad"] - HALO, tx * Tt * case["stride"] - case["pad"] - HALO
    tile = (g["b"] * tiles_y + ty) * tiles_x + tx
    z = lambda *s: np.zeros(s)
    dx, dxa, far, fara = z(B * H * W, C), z(B * H * W, C), z(B * H * W, C), z(B * H * W, C)
    n, n_win, n_far = z(B * H * W), z(B * H * W), z(B * H * W)
    win = z(B * tiles_y * tiles_x * WIN * WIN, C) if windows else None
    sides = np.zeros((2, M, T), bool)
    for k, (a, bb) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        ok = g["ok"][k]
        contrib = (g["wt"][k] * mk)[..., None] * G
        ry, rx = g["h0"] + a - y0[:, None], g["w0"] + bb - x0[:, None]
        inwin = ok & (ry >= 0) & (ry < WIN) & (rx >= 0) & (rx < WIN)
        isfar = ok & ~inwin
        sides[0] |= inwin
        sides[1] |= isfar
        np.add.at(dx, flat[k][ok], contrib[ok])
        np.add.at(dxa, flat[k][ok], np.abs(contrib[ok]))
        np.add.at(n, flat[k][ok], 1)
        np.add.at(far, flat[k][isfar], contrib[isfar])
        np.add.at(fara, flat[k][isfar], np.abs(contrib[isfar]))
        np.add.at(n_win, flat[k][inwin], 1)
        np.add.at(n_far, flat[k][isfar], 1)
        if windows:
            widx = (tile[:, None] * WIN + ry) * WIN + rx
            np.add.at(win, widx[inwin], contrib[inwin])
    sh4, sh3 = (B, H, W, C), (B, H, W)
    out.update(dx=dx.reshape(sh4), dx_abs=dxa.reshape(sh4), dx_n=n.reshape(sh3), dx_far=far.reshape(sh4), far_abs=fara.reshape(sh4),
               n_win=n_win.reshape(sh3), n_far=n_far.reshape(sh3), straddle=int((sides[0] & sides[1]).sum()))
    if windows:
        out["win"] = win.reshape(B * tiles_y * tiles_x, WIN, WIN, C)
    return out


def fixed_exponent(dcols):
    """e with 2^e > max |dcols| strictly (e = floor(log2 max) + 1), None for an all-zero array"""
    mx = float(np.abs(dcols).max())
    return None if mx == 0 else math.frexp(mx)[1]            # mx = f 2^e with 0.5 <= f < 1


def bounds(case, ref, const=None):
    """per-element bounds of every output, with `const` in place of CONST (the host test passes the ceilings)"""
    c = CONST if const is None else const
    b = {"cols": bf16_store(ref["cols"]) + c["CORNER"] * F32 * ref["cols_abs"]}
    if "dx" in ref:
        b["dmask"] = c["CH"] * F32 * ref["dmask_abs"]
        b["doffset"] = c["CH"] * F32 * ref["doffset_abs"]
        b["dx"] = c["DX"] * F32 * ref["dx_abs"]
        unit = 0.0 if ref["e"] is None else 2.0 ** (ref["e"] - 20)
        b["dx_tiled"] = bf16_store(ref["dx"]) + ref["n_win"][..., None] * unit + c["DX"] * F32 * ref["dx_abs"]
    return b


def bound_terms(case, ref):
    """(base, {constant: term}) per output, for the calibrating check of the GPU test"""
    unit = 0.0 if ref.get("e") is None else 2.0 ** (ref["e"] - 20)
    t = {"cols": (bf16_store(ref["cols"]), {"CORNER": F32 * ref["cols_abs"]})}
    if "dx" in ref:
        t["dmask"] = (np.zeros_like(ref["dmask"]), {"CH": F32 * ref["dmask_abs"]})
        t["doffset"] = (np.zeros_like(ref["doffset"]), {"CH": F32 * ref["doffset_abs"]})
        t["dx"] = (np.zeros_like(ref["dx"]), {"DX": F32 * ref["dx_abs"]})
        t["dx_tiled"] = (bf16_store(ref["dx"]) + ref["n_win"][..., None] * unit, {"DX": F32 * ref["dx_abs"]})
    return t


def im2col(case, x):
    """the ordinary im2col of x [B, H, W, C] (zero padding), [M, T C]: what the gather gives with offset = mask = NULL, to the bit"""
    B, H, W, C, s = case["B"], case["H"], case["W"], case["C"], case["stride"]
    xp = np.zeros((B, H + 2, W + 2, C), x.dtype)
    xp[:, 1:-1, 1:-1] = x
    cols = np.empty((B, case["Ho"], case["Wo"], 9, C), x.dtype)
    for t in range(9):
        i, j = divmod(t, 3)
        cols[:, :, :, t] = xp[:, i:i + s * case["Ho"]:s, j:j + s * case["Wo"]:s][:, :case["Ho"], :case["Wo"]]
    return cols.reshape(case["M"], 9 * C)


# ---- runners (C ABI; every output NaN-filled with GUARD elements after it) ----------------------------------------------------------------
def nan_buf(n, dtype, device="cuda"):
    t = torch.empty(n, dtype=dtype, device=device)
    (t.view(torch.int16) if dtype == torch.bfloat16 else t.view(torch.int32)).fill_(NAN_BF16 if dtype == torch.bfloat16 else NAN_F32)
    return t


def to_device(inp, device="cuda"):
    d = dict(x=torch.from_numpy(inp["x"]).to(torch.bfloat16).to(device).contiguous(),
             dcols=torch.from_numpy(inp["dcols"]).to(torch.bfloat16).to(device).contiguous())
    d["offset"] = None if inp["offset"] is None else torch.from_numpy(inp["offset"]).to(device)
    d["mask"] = None if inp["mask"] is None else torch.from_numpy(inp["mask"]).to(device)
    return d


def _dims(case):
    return tuple(case[k] for k in ("B", "H", "W", "C", "Ho", "Wo", "kh", "kw", "stride", "pad"))


def run_gather(lib, case, dev):
    cols = nan_buf(case["M"] * case["T"] * case["C"] + GUARD, torch.bfloat16)
    P = lib.ptr
    lib.call("fiber_dcn_gather_bf16", P(dev["x"]), P(dev["offset"]), P(dev["mask"]), P(cols), *_dims(case))
    return {"cols": cols}


def run_scatter(lib, case, dev, want=("dx", "doffset", "dmask")):
    """dx is accumulated into: zeroed here (its guard stays NaN)"""
    n = dict(dx=case["B"] * case["H"] * case["W"] * case["C"], doffset=case["M"] * 2 * case["T"], dmask=case["M"] * case["T"])
    o = {k: nan_buf(n[k] + GUARD, torch.float32) for k in want}
    if "dx" in o:
        o["dx"][:n["dx"]].zero_()
    P = lib.ptr
    lib.call("fiber_dcn_scatter_bf16", P(dev["dcols"]), P(dev["x"]), P(dev["offset"]), P(dev["mask"]), P(o.get("dx")), P(o.get("doffset")),
             P(o.get("dmask")), *_dims(case))
    return o


def run_tiled(lib, case, dev):
    """workspace: the windows NaN-filled (the kernels must write every word they later read), the `far` map and the scale word zero as
    the contract asks, GUARD words after it"""
    words = lib.plain("fiber_dcn_dx_workspace", case["B"], case["H"], case["W"], case["C"], case["Ho"], case["Wo"], case["stride"])
    assert words == workspace_words(case), (words, workspace_words(case))
    zero = case["B"] * case["H"] * case["W"] * case["C"] + 4
    ws = nan_buf(words + GUARD, torch.float32)
    ws[words - zero:words].zero_()
    n = case["B"] * case["H"] * case["W"] * case["C"]
    dx = nan_buf(n + GUARD, torch.bfloat16)
    P = lib.ptr
    lib.call("fiber_dcn_dx_bf16", P(dev["dcols"]), P(dev["offset"]), P(dev["mask"]), P(dx), P(ws), *_dims(case))
    return {"dx": dx, "ws": ws, "words": words, "zero": zero}
