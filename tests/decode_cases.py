"""Case table and fp64 reference of the single-token decode attention (csrc/attn_decode.hip; ops.mha_decode_self / ops.mha_decode_cross),
shared by tests/test_caption_decode_host.py (the torch restatements) and tests/test_hip_caption_decode.py (the kernels).

The reference is attn_cases.attention64 on one query row per (row, head), with the ancestry gather applied to K / V first; the bound is
its terms["O"] with attn_cases.CONST unchanged: U |O| + TINY + C_PV o_pv + C_S o_s."""
import torch

from tests import attn_cases as ac

# self-attention: position t of Lmax; t = 15 / 16 / 17 straddle one D = 64 lane group's keys, 49 is the named config's last step, 63 the limit
SELF_N = (1, 5, 6)
SELF_HEADS = (1, 2, 12)
SELF_T = (0, 1, 15, 16, 17, 49, 63)
# cross-attention: Lk = 9 / 49 / 144 / 324 occur; 1 is the smallest, 333 leaves a ragged sixth tile; R = 3, 5 sit between the register bounds
CROSS_G = (1, 3)
CROSS_R = (1, 3, 5, 8, 16)
CROSS_LK = (1, 9, 49, 144, 324, 333)
HEAD_DIMS = (32, 64)
PAD = 8                                                      # extra columns of every leading dimension, NaN-filled


def lmax_of(t):
    return 50 if t < 50 else 64


def gen(*key):
    return torch.Generator().manual_seed(1000003 * len(key) + sum((i + 1) * int(k) for i, k in enumerate(key)))


def make_self(N, heads, D, t, ancestry, dtype=torch.bfloat16):
    """-> dict(qkv [N, 3C] values, cache [N, Lmax, 2C] with positions < t random and the rest NaN, anc int32 [N, Lmax] or None), on the CPU,
    values exactly representable in bf16.  ancestry: False (anc None), True (a random valid ancestry) or "masked" (the same with about a
    third of the positions 1 .. t marked -1: padding under a key mask; position 0, the [CLS] of a caption, stays a key)"""
    C, Lmax = heads * D, lmax_of(t)
    g = gen(N, heads, D, t, len(str(ancestry)))
    qkv = torch.randn(N, 3 * C, generator=g).to(torch.bfloat16).to(dtype)
    cache = torch.full((N, Lmax, 2 * C), float("nan"), dtype=dtype)
    cache[:, :t] = torch.randn(N, t, 2 * C, generator=g).to(torch.bfloat16).to(dtype)
    anc = None
    if ancestry:
        anc = torch.full((N, Lmax), -7, dtype=torch.int32)  # entries past t are never read
        anc[:, :t] = torch.randint(0, N, (N, t), generator=g, dtype=torch.int32)
        anc[:, t] = torch.arange(N, dtype=torch.int32)
        if ancestry == "masked":
            drop = torch.rand(N, t + 1, generator=g) < 0.34
            drop[:, 0] = False
            anc[:, :t + 1][drop] = -1
    return dict(qkv=qkv, cache=cache, anc=anc, t=t, heads=heads, D=D, scale=D ** -0.5)


def gathered_cache(c):
    """The cache a physical reorder would have produced: row n holds, at every position j < t, what slot anc[n, j] holds"""
    if c["anc"] is None:
        return c["cache"].clone()
    t, N = c["t"], c["cache"].shape[0]
    out = c["cache"].clone()
    out[:, :t] = c["cache"][c["anc"][:, :t].long().clamp_min(0), torch.arange(t)[None, :].expand(N, t)]   # (a masked position: any finite row)
    return out


def live_keys(c):
    """bool [N, t + 1]: the positions that are keys (every one without an ancestry table)"""
    N, t = c["qkv"].shape[0], c["t"]
    if c["anc"] is None:
        return torch.ones(N, t + 1, dtype=torch.bool)
    a = c["anc"][:, :t + 1]
    return (a >= 0) & (a < N)


def self_reference(c):
    """-> (O [N, C] fp64, bound [N, C] fp64)"""
    t, heads, D = c["t"], c["heads"], c["D"]
    C, N = heads * D, c["qkv"].shape[0]
    past = gathered_cache(c)[:, :t].double()
    qkv = c["qkv"].double()
    kv = torch.cat([past, qkv[:, None, C:]], 1)                                # [N, t + 1, 2C]
    q = qkv[:, :C].view(N, 1, heads, D).transpose(1, 2)                          # [N, heads, 1, D]
    k = kv[..., :C].reshape(N, t + 1, heads, D).transpose(1, 2)
    v = kv[..., C:].reshape(N, t + 1, heads, D).transpose(1, 2)
    add = torch.zeros(N, t + 1, dtype=torch.float64).masked_fill(~live_keys(c), float("-inf"))
    return _one_row(q, k, v, c["scale"], add[:, None, None, :])


def make_cross(G, R, Lk, D, heads=None, spike=None, dtype=torch.bfloat16):
    """-> dict(q [G * R, C], kv [G, Lk, 2C]) on the CPU.  spike: "first" / "last": scores spanning about +-60 with the maximum on the first or
    the last key (attn_cases._spike's construction)"""
    heads = heads or (12 if D == 64 else 4)
    C = heads * D
    g = gen(G, R, Lk, D, heads, 0 if spike is None else len(spike))
    q = torch.randn(G, R, heads, D, generator=g)
    k = torch.randn(G, Lk, heads, D, generator=g)
    v = torch.randn(G, Lk, heads, D, generator=g)
    if spike is not None:
        q[..., 1:] *= 0.25
        k[..., 1:] *= 0.25
        pos = torch.arange(Lk)[None, :, None].expand(G, Lk, heads)
        ac._spike(q, k, pos, Lk, spike == "first", D ** -0.5)
    kv = torch.cat([k.reshape(G, Lk, C), v.reshape(G, Lk, C)], -1).to(torch.bfloat16).to(dtype)
    return dict(q=q.reshape(G * R, C).to(torch.bfloat16).to(dtype), kv=kv, R=R, heads=heads, D=D, scale=D ** -0.5)


def cross_reference(c):
    """-> (O [N, C] fp64, bound [N, C] fp64)"""
    heads, D, R = c["heads"], c["D"], c["R"]
    G, Lk, C = c["kv"].shape[0], c["kv"].shape[1], heads * D
    q = c["q"].double().view(G, R, heads, D).transpose(1, 2)                     # [G, heads, R, D]: R query rows against the image's keys
    k = c["kv"][..., :C].double().reshape(G, Lk, heads, D).transpose(1, 2)
    v = c["kv"][..., C:].double().reshape(G, Lk, heads, D).transpose(1, 2)
    return _one_row(q, k, v, c["scale"])


def _one_row(q, k, v, scale, add=None):
    G, heads, Lq, D = q.shape
    if add is None:
        add = torch.zeros(1, 1, Lq, k.shape[2], dtype=torch.float64)
    out, terms = ac.attention64(q, k, v, add, torch.zeros_like(q), scale)
    base, parts = terms["O"]
    bound = base + sum(ac.CONST[c] * x for c, x in parts.items())
    rows = lambda x: x.transpose(1, 2).reshape(G * Lq, heads * D)
    return rows(out["O"]), rows(bound)


def padded(x, fill=float("nan")):
    """[rows, cols] -> a [rows + 1, cols + PAD] buffer of `fill` holding x in its corner (a guard row, PAD guard columns)"""
    buf = torch.full((x.shape[0] + 1, x.shape[1] + PAD), fill, dtype=x.dtype, device=x.device)
    buf[:-1, :x.shape[1]] = x
    return buf
