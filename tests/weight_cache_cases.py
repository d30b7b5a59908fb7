"""The derived weight copies of fiber_amd/ops.py (`_wcache`, `_packs`) against what they are copies OF.

Every kind of copy has its expected value here as a plain torch expression of the fp32 master(s); the index permutations are
restated from the layout comments, nothing is imported from ops.py for them.  All comparisons are torch.equal -- a copy is a
cast / permutation / fold of the master, so there is no tolerance to give.  (The folded fc1 bias b1 + W1.beta stays fp32: the
expected value is the same torch.addmv on the same device, fp32 summation order being part of the op.)

`audit(params)` walks both caches: an entry whose stamp says "current" must HOLD the expected value; an entry whose stamp says
"stale" must be REPLACED by the expected value at the next accessor call.  It returns the kinds it saw, so that a test can
assert that it exercised what it claims to.

The cases (`make_cases`) are the smallest shapes that still take every branch of the cache code; `run()` is the consuming op,
forward and backward, on the GPU, and the bare accessor calls on the host (the consumers are HIP kernels)."""
import torch

BF = torch.bfloat16

PLAIN_KINDS = ("plain", "T", "HM", "pack")          # rewritten by FiberAdamW.step() itself
LAZY_KINDS = ("LNMLP", "pe", "KC", "KCT", "V2plain")   # rebuilt by the next forward pass


# ---- expected values --------------------------------------------------------------------------------------------------------
def qkv_perm(C, heads, device="cpu"):
    """Head-major output order [heads][3][32]: row h*96 + which*32 + d of the copy is row which*C + h*32 + d of qkv.weight."""
    return torch.tensor([which * C + h * 32 + d for h in range(heads) for which in range(3) for d in range(32)], device=device)


def k_swap(K, device="cpu"):
    """The K order of the fused LayerNorm-Mlp kernel's operands: position p holds index p with bits 2 and 3 exchanged."""
    return torch.tensor([(i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1) for i in range(K)], device=device)


def exp_plain(w):
    return w.detach().to(BF)


def exp_t(w):
    return exp_plain(w).t()


def exp_hm(w, b, heads):
    p = qkv_perm(w.shape[1], heads, w.device)
    wp = w.detach()[p].to(BF)
    return wp, b.detach()[p], wp.t()


def exp_pack(ws, bs):
    plain = torch.cat([w.detach().to(BF) for w in ws], 0)
    return plain, plain.t(), (torch.cat([b.detach().reshape(-1) for b in bs]) if bs[0] is not None else None)


def exp_lnmlp(gamma, beta, w1, b1, w2):
    """(w1p, b1p, w2p, w2tp, w1tp): W1 diag(gamma) and b1 + W1 beta in fp32, one rounding; K = hidden copies in the kernel's order."""
    w1f = w1.detach().float()
    w1p = (w1f * gamma.detach().float()[None, :]).to(BF)
    b1p = torch.addmv(b1.detach().float(), w1f, beta.detach().float())
    w2b = w2.detach().to(BF)
    sw = k_swap(w1.shape[0], w1.device)
    return w1p, b1p, w2b[:, sw], w2b.t(), w1p.t()[:, sw]


def exp_pe(w):
    out = torch.zeros((w.shape[0], 64), dtype=BF, device=w.device)
    out[:, :48] = w.detach().reshape(w.shape[0], 48).to(BF)
    return out


def exp_kc(w):
    Cout = w.shape[0]
    rows = w.detach().permute(0, 2, 3, 1).reshape(Cout, -1).to(BF)            # tap-major: (ky, kx, cin)
    out = torch.zeros((-(-Cout // 8) * 8, rows.shape[1]), dtype=BF, device=w.device)
    out[:Cout] = rows
    return out


def exp_kct(w):
    return exp_kc(w).t()


def _same(name, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype and got.device == want.device, \
        f"{name}: {tuple(got.shape)} {got.dtype} {got.device} for {tuple(want.shape)} {want.dtype} {want.device}"
    assert got.is_contiguous(), f"{name}: copy is not contiguous"
    if not torch.equal(got, want):
        bad = (got != want)
        raise AssertionError(f"{name}: {int(bad.sum())} of {got.numel()} elements differ from the expected copy of the master "
                             f"(max |diff| {float((got.float() - want.float()).abs().max()):.3g})")


# ---- composites: which parameters belong together -----------------------------------------------------------------------------
class HM:
    def __init__(self, w, b, heads):
        self.w, self.b, self.heads = w, b, heads


class LNMLP:
    def __init__(self, gamma, beta, w1, b1, w2):
        self.five = (gamma, beta, w1, b1, w2)


class Pack:
    def __init__(self, ws, bs):
        self.ws, self.bs = list(ws), list(bs)


class PE:
    def __init__(self, w, b):
        self.w, self.b = w, b


def _touch_hm(ops, s):
    if not s.w.is_cuda:                                  # (the op is a HIP kernel: on the host, its accessor)
        return ops._head_major_weights(s.w, s.b, s.heads)
    with torch.no_grad():
        ops.linear_qkv_head_major(torch.zeros(64, s.w.shape[1], dtype=BF, device=s.w.device), s.w, s.b, s.heads)


def _touch_pe(ops, s):
    if not s.w.is_cuda:
        return ops._patch_embed_weight(s.w)
    with torch.no_grad():
        ops.patch_embed_proj(torch.zeros(1, 3, 32, 32, device=s.w.device), s.w, s.b)


def audit(params, ops=None, accessors=True):
    """See the module docstring.  `params`: parameters and HM / LNMLP / Pack / PE groups (an entry of a composite kind whose group
    is not given is checked through the members the entry itself remembers, where it remembers them).  accessors=False: stale
    entries are left alone (the graph-replay test looks at the cache as the replay left it)."""
    if ops is None:
        from fiber_amd import ops
    hm = {id(s.w): s for s in params if isinstance(s, HM)}
    ln = {id(s.five[2]): s for s in params if isinstance(s, LNMLP)}
    pe = {id(s.w): s for s in params if isinstance(s, PE)}
    packs = {tuple(id(w) for w in s.ws): s for s in params if isinstance(s, Pack)}
    seen = set()
    views = {id(v[1]) for k, v in ops._wcache.items() if isinstance(k, tuple) and k[0] == "V2"}
    for key in list(ops._wcache):
        ent = ops._wcache.get(key)
        if ent is None:
            continue
        stamp, val, ref = ent
        w = ref()
        if w is None:
            continue
        kind = key[0] if isinstance(key, tuple) else ("V2plain" if key in views else "plain")
        name = f"{kind} copy of {tuple(w.shape)}"
        if kind in ("plain", "V2plain", "T", "KC", "KCT"):
            want, get = {"plain": (exp_plain, ops.bf16_weight), "V2plain": (exp_plain, ops.bf16_weight), "T": (exp_t, ops.bf16_weight_t),
                         "KC": (exp_kc, ops._conv_weight_rows),
                         "KCT": (exp_kct, lambda t: ops._conv_weight_rows(t, transposed=True))}[kind]
            if stamp != ops._stamp(w) or val.device != w.device:
                if not accessors:
                    continue
                val = get(w)
                name += " (rebuilt by its accessor)"
                assert ops._cache_get(key, w)[0] == ops._stamp(w), name + ": not marked current after the accessor call"
            _same(name, val, want(w).contiguous())
        elif kind == "V2":
            if val.data_ptr() != w.data_ptr():
                if not accessors:
                    continue
                val = ops._weight_2d(w)
            assert val.data_ptr() == w.data_ptr() and val.shape == w.shape[:2] and val._version == w._version, name + ": not a view of the parameter"
            assert torch.equal(val, w.detach().reshape(w.shape[0], w.shape[1])), name
        elif kind == "pe":
            s = pe.get(id(w))
            if stamp != ops._stamp(w):
                if not accessors or s is None:
                    continue
                _touch_pe(ops, s)
                val = ops._wcache[key][1]
                name += " (rebuilt by the next forward)"
            _same(name, val, exp_pe(w))
        elif kind == "HM":
            s = hm.get(id(w))
            b, heads = (s.b, s.heads) if s is not None else (val[3](), val[4])
            if b is None:
                continue
            if stamp != (ops._stamp(w), ops._stamp(b)) or val[3]() is not b:
                if not accessors:
                    continue
                _touch_hm(ops, s if s is not None else HM(w, b, heads))
                val = ops._wcache[key][1]
                name += " (rebuilt by the next forward)"
            for part, got, want in zip(("weight", "bias", "transpose"), val[:3], exp_hm(w, b, heads)):
                _same(f"{name}, {part}", got, want.contiguous())
        elif kind == "LNMLP":
            s = ln.get(id(w))
            five = s.five if s is not None else (tuple(r() for r in val[5]) if len(val) > 5 else None)
            if five is None or any(t is None for t in five):
                continue
            current = stamp == tuple(ops._stamp(t) for t in five) and (len(val) <= 5 or all(r() is t for r, t in zip(val[5], five)))
            if not current:
                if not accessors:
                    continue
                val = ops._ln_mlp_weights(*five)
                name += " (rebuilt by its accessor)"
            for part, got, want in zip(("w1p", "b1p", "w2p", "w2tp", "w1tp"), val[:5], exp_lnmlp(*five)):
                _same(f"{name}, {part}", got, want.contiguous())
        else:
            raise AssertionError(f"weight cache holds a kind of copy this audit does not know: {key!r}")
        seen.add(kind)
    for key in list(ops._packs):
        pk = ops._packs.get(key)
        ws = [r() for r in pk["refs"]] if pk is not None else [None]
        if any(w is None for w in ws):
            continue
        s = packs.get(key)
        if s is None:
            continue                                     # (the biases are not remembered by the pack itself)
        name = f"pack of {len(ws)} x {tuple(ws[0].shape)}"
        hits = [ops._cache_get(id(w), w) for w in ws]
        stamps = tuple(ops._stamp(w) for w in ws)
        current = all(h is not None and h[0] == st for h, st in zip(hits, stamps)) and pk["t_stamp"] == stamps
        if s.bs[0] is not None:
            current = current and pk["bias"] is not None and all(
                b.data_ptr() == pk["bias"].data_ptr() + 4 * off for b, off in zip(s.bs, _offsets(pk["Ns"])))
        if not current:
            if not accessors:
                continue
            ops._pack_get(s.ws, s.bs)
            pk = ops._packs[key]
            name += " (refreshed by its accessor)"
            assert pack_is_current(ops, s), name + ": not marked current after the accessor call"
        plain, t, bias = exp_pack(s.ws, s.bs)
        _same(name + ", plain", pk["plain"], plain)
        _same(name + ", transpose", pk["t"], t.contiguous())
        for w, off, n in zip(s.ws, _offsets(pk["Ns"]), pk["Ns"]):
            view = ops._cache_get(id(w), w)[1]
            assert view.data_ptr() == pk["plain"].data_ptr() + 2 * off * pk["K"] and view.shape == (n, pk["K"]), \
                name + ": a member's working copy is not a row view of the packed buffer"
        if bias is not None:
            _same(name + ", bias", pk["bias"], bias)
            for b, off in zip(s.bs, _offsets(pk["Ns"])):
                assert b.data_ptr() == pk["bias"].data_ptr() + 4 * off, name + ": a member's bias is not a slice of the packed bias"
        seen.add("pack")
    return seen


def entry_pairs(ops, key, ent, biases=None, m=lambda t: t):
    """[(cached tensor, expected tensor)] of one `_wcache` entry, the expected values formed from m(master) instead of the master
    itself (m: a look-up of earlier values of the same parameters).  Members of composite entries are those the entry remembers.
    None for an entry whose owner is gone, and for the 2-D views (they hold no copy)."""
    stamp, val, ref = ent
    w = ref()
    kind = key[0] if isinstance(key, tuple) else "plain"
    if w is None or kind == "V2":
        return None
    if kind == "HM":
        want = exp_hm(m(w), m(val[3]()), val[4])
        return list(zip(val[:3], want))
    if kind == "LNMLP":
        return list(zip(val[:5], exp_lnmlp(*(m(r()) for r in val[5]))))
    fn = {"plain": exp_plain, "T": exp_t, "KC": exp_kc, "KCT": exp_kct, "pe": exp_pe}[kind]
    return [(val, fn(m(w)))]


def pairs_equal(pairs):
    return all(torch.equal(a, b.contiguous()) for a, b in pairs)


def _offsets(ns):
    out, off = [], 0
    for n in ns:
        out.append(off)
        off += n
    return out


def is_current(ops, key, w, extra=None):
    """Does the entry's own stamp call it current (without touching it)?"""
    ent = ops._cache_get(key, w)
    if ent is None:
        return False
    if isinstance(key, tuple) and key[0] == "HM":
        return ent[0] == (ops._stamp(w), ops._stamp(extra)) and ent[1][3]() is extra
    return ent[0] == ops._stamp(w)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def _p(gen, *shape, std=0.5, device="cpu"):
    return torch.nn.Parameter((torch.randn(*shape, generator=gen) * std).to(device))


class Case:
    """params: every fp32 master (an nn.ParameterList, so that load_state_dict is the module's own); groups: what audit() needs;
    kinds: the kinds of copy one run() leaves in the cache; fast: (key, parameter, extra) of the entries FiberAdamW.step() rewrites
    itself; slow: ... of those it leaves to the lazy path although they are of a kind it rewrites (odd shapes)."""

    def __init__(self, name, params, groups, kinds, run, host, fast=(), slow=(), launches=()):
        self.name, self.params, self.groups, self.kinds = name, torch.nn.ParameterList(params), list(groups), set(kinds)
        self.run, self.host, self.fast, self.slow, self.launches = run, host, list(fast), list(slow), set(launches)

    def audit_args(self):
        return list(self.params) + self.groups


def make_cases(device, names=None):
    """name -> Case on `device`.  On the host run is None (the consumers are HIP kernels) and host() calls the bare accessors."""
    from fiber_amd import ops
    gpu = torch.device(device).type == "cuda"
    g = torch.Generator().manual_seed(1234)
    out = {}

    def xin(*shape):
        return (torch.randn(*shape, generator=g)).to(BF).to(device).requires_grad_(True)

    def fb(fn, x):                                      # forward + backward; the output gradient is fixed by the output's shape
        y = fn(x)
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(y.numel())).to(y.dtype).to(device)
        x.grad = None
        y.backward(gy)
        return y.detach().clone(), (x.grad.clone() if x.grad is not None else None)

    def linear(name, N, K):
        w, b = _p(g, N, K, device=device), _p(g, N, device=device)
        x = xin(37, K)
        def host():
            ops.bf16_weight(w), ops.bf16_weight_t(w)
        out[name] = Case(name, [w, b], [], {"plain", "T"}, (lambda: fb(lambda x_: ops.linear(x_, w, b), x)) if gpu else None, host,
                         fast=[(id(w), w, None), (("T", id(w)), w, None)], launches={"fiber_transpose_multi_bf16"})
    linear("linear64", 64, 64)
    linear("linear40x24", 40, 24)

    # 20 x 12: no dimension a multiple of 8 -- no tile kernel takes such a weight (ops.linear sends it to the library GEMM, which
    # keeps no copy), so only the accessors are called; the one-launch transpose skips it and the lazy path alone serves it
    w_odd = _p(g, 20, 12, device=device)
    def odd_host():
        ops.bf16_weight(w_odd), ops.bf16_weight_t(w_odd)
    out["odd20x12"] = Case("odd20x12", [w_odd], [], {"plain", "T"}, None, odd_host, fast=[(id(w_odd), w_odd, None)],
                           slow=[(("T", id(w_odd)), w_odd, None)])

    # fused LayerNorm-Mlp at C = 128 (the only width the fused kernel is used at)
    C = 128
    five = (_p(g, C, device=device), _p(g, C, device=device), _p(g, 4 * C, C, std=C ** -0.5, device=device),
            _p(g, 4 * C, device=device), _p(g, C, 4 * C, std=(4 * C) ** -0.5, device=device))
    b2 = _p(g, C, device=device)
    xl = xin(100, C)
    out["lnmlp128"] = Case("lnmlp128", list(five) + [b2], [LNMLP(*five)], {"LNMLP"},
                           (lambda: fb(lambda x_: ops.ln_mlp(x_, five[0], five[1], 1e-5, five[2], five[3], five[4], b2), xl)) if gpu else None,
                           lambda: ops._ln_mlp_weights(*five))

    def conv(name, Cout):
        w, b = _p(g, Cout, 16, 3, 3, std=0.1, device=device), _p(g, Cout, device=device)
        x = xin(2, 5, 7, 16)
        def host():
            ops._conv_weight_rows(w), ops._conv_weight_rows(w, transposed=True)
        out[name] = Case(name, [w, b], [], {"KC", "KCT"}, (lambda: fb(lambda x_: ops.deform_conv(x_, None, None, w, b, 1, 1), x)) if gpu else None, host)
    conv("conv27", 27)
    conv("conv16", 16)

    wv, bv = _p(g, 32, 16, 1, 1, device=device), _p(g, 32, device=device)
    xv = xin(2, 5, 7, 16)
    def v2_host():
        v = ops._weight_2d(wv)
        ops.bf16_weight(v), ops.bf16_weight_t(v)
    out["conv1x1"] = Case("conv1x1", [wv, bv], [], {"V2", "V2plain", "T"}, (lambda: fb(lambda x_: ops.conv1x1(x_, wv, bv), xv)) if gpu else None, v2_host)

    Cq, heads = 64, 2
    wq, bq = _p(g, 3 * Cq, Cq, std=Cq ** -0.5, device=device), _p(g, 3 * Cq, device=device)
    xq = xin(2, 9, Cq)
    out["qkv64"] = Case("qkv64", [wq, bq], [HM(wq, bq, heads)], {"HM"}, (lambda: fb(lambda x_: ops.linear_qkv_head_major(x_, wq, bq, heads), xq)) if gpu else None,
                        lambda: ops._head_major_weights(wq, bq, heads), fast=[(("HM", id(wq)), wq, bq)], launches={"fiber_rowperm_cast_multi_bf16"})

    ws = [_p(g, 64, 64, std=0.125, device=device) for _ in range(3)]
    bs = [_p(g, 64, device=device) for _ in range(3)]
    xp = xin(37, 64)
    out["pack3"] = Case("pack3", ws + bs, [Pack(ws, bs)], {"pack", "plain"},
                        (lambda: fb(lambda x_: ops.linear_packed(x_, list(zip(ws, bs))), xp)) if gpu else None, lambda: ops._pack_get(ws, bs),
                        fast=[(id(w), w, None) for w in ws], launches={"fiber_transpose_multi_bf16"})

    wpe, bpe = _p(g, 32, 3, 4, 4, device=device), _p(g, 32, device=device)
    img = torch.randn(2, 3, 8, 8, generator=g).to(device)
    def pe_run():
        y = ops.patch_embed_proj(img, wpe, bpe)
        y.backward(torch.ones_like(y))
        return y.detach().clone(), None                  # the image is data: there is no input gradient
    out["patch_embed"] = Case("patch_embed", [wpe, bpe], [PE(wpe, bpe)], {"pe"}, pe_run if gpu else None, lambda: ops._patch_embed_weight(wpe))
    if names is not None:
        out = {k: out[k] for k in names}
    return out


GPU_CASES = ("linear64", "linear40x24", "odd20x12", "lnmlp128", "conv27", "conv16", "conv1x1", "qkv64", "pack3", "patch_embed")
HOST_CASES = GPU_CASES                               # every kind has a plain-torch accessor: all of them run on the host too


def pack_is_current(ops, s):
    pk = ops._packs.get(tuple(id(w) for w in s.ws))
    if pk is None:
        return False
    stamps = tuple(ops._stamp(w) for w in s.ws)
    return pk["t_stamp"] == stamps and all(is_current(ops, id(w), w) for w in s.ws)


# ---- the writers ------------------------------------------------------------------------------------------------------------
def _new_values(p, k=0):
    gen = torch.Generator().manual_seed(977 + p.numel() + k)
    return (torch.randn(p.shape, generator=gen) * 0.3).to(p.device)


def w_copy(case):
    with torch.no_grad():
        for p in case.params:
            p.copy_(_new_values(p))


def w_mul(case):
    with torch.no_grad():
        for p in case.params:
            p.mul_(1.5)


def w_load_state_dict(case):
    case.params.load_state_dict({k: _new_values(v, 1) for k, v in case.params.state_dict().items()})


def _give_grads(case):
    for i, p in enumerate(case.params):
        p.grad = _new_values(p, 10 + i)


def _torch_adamw(case, **kw):
    from fiber_amd import ops
    _give_grads(case)
    opt = torch.optim.AdamW(list(case.params), lr=1e-2, **kw)
    opt.register_step_post_hook(lambda *a, **k: ops.mark_weights_dirty())       # as fiber_utils.set_schedule registers it
    opt.step()


def w_adamw_foreach(case):
    _torch_adamw(case, foreach=True)


def w_adamw_fused(case):
    _torch_adamw(case, fused=True)


def w_data_new_values(case):
    for p in case.params:
        p.data = _new_values(p, 2)


def w_data_moved(case):
    for p in case.params:
        p.data = p.data.clone()


def w_data_inplace_then_dirty(case):
    from fiber_amd import ops
    for p in case.params:
        p.data.mul_(2.0)
    ops.mark_weights_dirty()


HOST_WRITERS = {"copy_": w_copy, "mul_": w_mul, "load_state_dict": w_load_state_dict, "adamw_foreach": w_adamw_foreach,
                "data_new_values": w_data_new_values, "data_moved": w_data_moved, "data_inplace_dirty": w_data_inplace_then_dirty}
# writers after which every copy must be STALE by its stamp (data_moved: same values, but nothing says so)
GPU_WRITERS = dict(HOST_WRITERS, adamw_fused=w_adamw_fused)
