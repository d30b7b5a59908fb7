"""Element-wise, cross-entropy and embedding kernel paths (csrc/elementwise.hip, loss.hip, embed.hip): the host restatement of the
dropout / DropPath hashes, fp64 references on the kernels' own rounded inputs, and the per-element bounds.

Bounds (|got - ref| per element) follow tests/norm_cases.py: a bf16 store term 2^-8 |ref| where the kernel stores bf16, plus a constant
of CONST times a scale of the fp32 arithmetic -- sum |terms| for column sums, dots, folds and the embedding LayerNorm, (1 + |lse|) for the
log-sum-exp.  Each constant is the smallest power of two that passes every case on MI355X (tests/test_hip_ew_paths.py with
FIBER_EW_CALIBRATE=<file> writes what each constant needed).  The dropout and DropPath masks are not bounded: they must match the
restatement below element by element."""
import numpy as np
import torch

# fp32 arithmetic terms, needed on MI355X in brackets (the largest |err| - other terms, over sum |terms|, of any element of any case)
CONST = {
    "EW": 2.0 ** -22,      # single-pass fp32 element-wise math: stream_add, scale_add, rowscale_add, dropout, casts (2^-22.66, stream_add o32)
    "SUM": 2.0 ** -20,     # fp32 column sums / dots / folds, in units of sum |terms| (2^-20.87, colsum_labelled V = 50265: up to
                           # 256 sequential adds per column accumulator; the slab column sums and folds needed 2^-22.31)
    "LSE": 2.0 ** -23,     # cross-entropy lse and loss, in units of (1 + |lse| + |x[label]|) (2^-23.47, lse V = 50265)
    "EXP": 2.0 ** -23,     # cross-entropy backward: exp(x - lse), in units of p (1 + |x| + |lse|).  Not calibrated: no element needed more
                           # than the bf16 store term, so this is a chosen allowance for __expf (a few ulp), not a measured need
    "EMB": 2.0 ** -22,     # embedding LayerNorm forward and backward, in units of its |terms| (2^-22.79, dword C = 768)
}
EXP_FLOOR = 2.0 ** -125    # __expf flushes results below the smallest normal fp32 to zero: an absolute floor, times the scale
BF16_STORE = 2.0 ** -8     # a bf16 store: half an ulp is 2^-8 |v| at most (7 stored mantissa bits), relative to |ref|
GELU_BWD_ERR = 2.0 ** -12  # |gelu'_poly - gelu'| of the backward's minimax polynomial (1.7e-4 measured, common.h), times |dg|
NAN_BF16 = 0x7FC0
NAN_F32 = 0x7FC00000
M32 = 0xFFFFFFFF
_K1, _K2 = 0x9E3779B1, 0x7FEB352D


# ---- the hashes of csrc/common.h, in numpy uint32 / uint64 --------------------------------------------------------------------------
def fmix32(x):
    x = np.asarray(x, dtype=np.uint32)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x85EBCA6B)
        x = x ^ (x >> np.uint32(13))
        x = x * np.uint32(0xC2B2AE35)
        x = x ^ (x >> np.uint32(16))
    return x


def drop_seed32(seed):
    seed = int(seed) & ((1 << 64) - 1)
    return np.uint32(((seed & M32) ^ (((seed >> 32) * _K1) & M32)) & M32)


def drop_base(seed, base):
    """drop_base(seed, base) for an array of (uint64) base indices"""
    base = np.asarray(base, dtype=np.uint64)
    lo = (base & np.uint64(M32)).astype(np.uint32)
    hi = (base >> np.uint64(32)).astype(np.uint32)
    with np.errstate(over="ignore"):
        return drop_seed32(seed) + lo * np.uint32(_K1) + hi * np.uint32(_K2)


def drop_keep_e(h0, e, thresh):
    with np.errstate(over="ignore"):
        return fmix32(np.asarray(h0, dtype=np.uint32) + np.uint32(e) * np.uint32(_K1)) >= np.uint32(thresh)


def thresh_of(p):
    """(uint32)((double)p * 2^32) of the fp32 probability the ABI receives"""
    return int(float(np.float32(p)) * 4294967296.0)


def inv_keep(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_mask(seed, n, p, group=8):
    """keep decision of flat element i = 0..n-1 as the kernels draw it: vectors of `group` elements share drop_base(seed, first index)"""
    i = np.arange(n, dtype=np.uint64)
    first = i - (i % np.uint64(group))
    return drop_keep_e(drop_base(seed, first), (i % np.uint64(group)).astype(np.uint32), thresh_of(p))


def hash_u32(seed, idx):
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & ((1 << 64) - 1)) + idx * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint32)


def droppath_scale(n, keep, seed):
    """fiber_droppath_scale_f32 in fp32: floor(keep + u) / keep with u = (h >> 9) 2^-23 < 1"""
    u = (hash_u32(seed, np.arange(n)) >> np.uint32(9)).astype(np.float32) * np.float32(1.0 / 8388608.0)
    k = np.float32(keep)
    return np.floor(k + u).astype(np.float32) / k


def seed_hitting_top(n_samples, lo=2 ** 32 - 128, start=1):
    """a seed whose DropPath draw of some sample has h >= lo (u = 1.0f under the old 32-bit draw): a host search"""
    s = start
    while True:
        h = hash_u32(s, np.arange(n_samples))
        hit = np.nonzero(h >= np.uint32(lo))[0]
        if hit.size:
            return s, int(hit[0])
        s += 1


# ---- fp64 references ----------------------------------------------------------------------------------------------------------------
def mask_t(seed, n, p, device, group=8):
    return torch.from_numpy(keep_mask(seed, n, p, group)).to(device)


def stream_add_ref(res, a, b, alpha, rs_elem, p_a, seed_a, p_b, seed_b):
    """(ref, sum |terms|) of res + rs * (drop_a(a) + alpha drop_b(b)), fp64, flat [n]; rs_elem: per-element factor or None"""
    n = a.numel()
    va = a.double()
    if p_a > 0:
        va = torch.where(mask_t(seed_a, n, p_a, a.device), va * inv_keep(p_a), torch.zeros_like(va))
    v, t = va, va.abs()
    if b is not None:
        vb = b.double()
        if p_b > 0:
            vb = torch.where(mask_t(seed_b, n, p_b, a.device), vb * inv_keep(p_b), torch.zeros_like(vb))
        al = 1.0 if alpha is None else float(alpha)
        v, t = v + al * vb, t + abs(al) * vb.abs()
    if rs_elem is not None:
        v, t = v * rs_elem, t * rs_elem.abs()
    if res is not None:
        v, t = v + res.double(), t + res.double().abs()
    return v, t


def colsum_ref(x):
    x = x.double()
    return x.sum(0), x.abs().sum(0)


def ce_ref(x, labels, ignore):
    """lse, loss (0 on ignored rows), pred (torch.argmax, -1 on ignored rows) of bf16 logits, fp64"""
    xd = x.double()
    lse = torch.logsumexp(xd, 1)
    ign = labels == ignore
    lab = labels.clamp(0, x.shape[1] - 1)
    picked = xd.gather(1, lab[:, None])[:, 0]
    loss = torch.where(ign, torch.zeros_like(lse), lse - picked)
    pred = torch.where(ign, torch.full_like(labels, -1), x.float().argmax(1))
    return lse, loss, pred, picked


def ce_bwd_ref(x, labels, lse, scale, ignore):
    """(exp(x - lse) - onehot) * scale with the kernel's own lse, and p = exp(x - lse); zero rows where ignored"""
    xd = x.double()
    p = torch.exp(xd - lse.double()[:, None])
    oh = torch.zeros_like(p)
    ign = labels == ignore
    oh[torch.arange(x.shape[0], device=x.device), labels.clamp(0, x.shape[1] - 1)] = 1.0
    g = (p - oh) * scale
    g[ign] = 0
    p = p.clone()
    p[ign] = 0
    return g, p


def roberta_positions(ids, pad):
    """RoBERTa create_position_ids_from_input_ids: cumsum(ids != pad) * (ids != pad) + pad"""
    m = (ids != pad).long()
    return torch.cumsum(m, 1) * m + pad


def embed_fwd_ref(ids, word, pos_tab, type_tab, gamma, beta, pad, eps):
    pos = roberta_positions(ids, pad)
    w, pp, t = word[ids].double(), pos_tab[pos].double(), type_tab[0].double()[None, None]
    x = w + t + pp
    A = (w.abs() + t.abs() + pp.abs())                            # scale of the fp32 three-term sum
    mu = x.mean(-1)
    var = ((x - mu[..., None]) ** 2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mu[..., None]) * rstd[..., None]
    y = xh * gamma.double() + beta.double()
    Arow = A.amax(-1)
    return dict(pos=pos, y=y, mean=mu, rstd=rstd, x=x, Arow=Arow)


def embed_bwd_ref(ids, pos, dy_eff, gamma, x, mean, rstd, n_word, n_pos, pad):
    """gradients of the word / position / type tables and gamma / beta from the kernel's own mean / rstd, fp64, with the |terms| of each"""
    C = x.shape[-1]
    xh = (x - mean.double()[..., None]) * rstd.double()[..., None]
    d = dy_eff.double()
    g = gamma.double()
    dg = d * g
    s1 = dg.mean(-1, keepdim=True)
    s2 = (dg * xh).mean(-1, keepdim=True)
    rs = rstd.double()[..., None]
    de = rs * (dg - s1 - xh * s2)
    tde = rs * (dg.abs() + s1.abs() + xh.abs() * s2.abs() + (dg.abs().mean(-1, keepdim=True) + (dg * xh).abs().mean(-1, keepdim=True) * xh.abs()))
    de2, t2 = de.reshape(-1, C), tde.reshape(-1, C)
    idf, psf = ids.reshape(-1), pos.reshape(-1).long()
    out = {}
    for name, key, nrows in (("dword", idf, n_word), ("dpos", psf, n_pos)):
        keep = key != pad
        ref = torch.zeros(nrows, C, dtype=torch.float64, device=x.device).index_add_(0, key[keep], de2[keep])
        term = torch.zeros_like(ref).index_add_(0, key[keep], t2[keep])
        out[name] = (ref, term)
    out["dtype"] = (de2.sum(0), t2.sum(0))
    d2, xh2 = d.reshape(-1, C), xh.reshape(-1, C)
    out["dgamma"] = ((d2 * xh2).sum(0), (d2 * xh2).abs().sum(0) + (d2.abs() * (xh2.abs() + 1)).sum(0))
    out["dbeta"] = (d2.sum(0), d2.abs().sum(0))
    return out


def im2col_ref(img):
    """[B,3,H,W] fp32 -> [B*(H/4)*(W/4), 64] bf16, column c*16 + kh*4 + kw, zeros in 48..63"""
    B, _, H, W = img.shape
    p = img.to(torch.bfloat16).reshape(B, 3, H // 4, 4, W // 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(-1, 48)
    return torch.cat([p, torch.zeros(p.shape[0], 16, dtype=torch.bfloat16, device=img.device)], 1)
