"""Case table of the autograd layer (fiber_amd/ops.py): one entry per torch.autograd.Function of the backbone, heads and losses, at the
smallest shapes that reach each branch of its forward / backward, with the plain operation in torch fp64 autograd as the reference.
Shared by tests/test_hip_autograd_graphs.py (the Functions on the GPU under graph variants: frozen inputs, forms of the incoming
gradient, outputs consumed twice or not at all, repeated passes) and tests/test_autograd_graphs_host.py (the bounds on the host).

What the kernels compute is pinned per element at the C ABI by the *_cases.py tables; this table pins what the Functions CHOOSE: which
kernels run, which gradients are skipped, which by-products are handed from one backward node to the next.  Those choices depend on the
shape of the graph, so every entry is a small graph whose leaves can be frozen one by one.

An entry has
  make(device)              -> Case: leaves {name: tensor} (bf16-exact values, so the fp64 reference reads what the kernels read), the
                               names that are parameters, extra (labels, DropPath factors, fp32 payloads ...), gs (one incoming gradient
                               per output)
  run(ops, L, E, mid)       -> outputs of the Function(s) on the leaves L (requires_grad set by the caller)
  ref(L, E, mid, rn)        -> the same outputs by the plain torch operation in the dtype of L (fp64: the reference; fp32 with rn = a
                               bf16 rounding that also rounds the gradient passing through it: the host emulation of the kernels)
  twin(L, E, gs, dmid)      -> {leaf: A}: the fp64 absolute twin of each gradient, the same sum over the magnitudes of its factors
`mid(t, f)` wraps the point where an intermediate tensor t (logits, qkv) is consumed by f: the graph tests hang a second consumer there.

Bound, per element (hip_util.assert_elementwise):   |got - ref| <= 2^-8 |ref| + CONST[family] * A + TINY
A carries the roundings INSIDE the graph: the bf16 stores of intermediates (pre-activation, gelu(H), dH, dlogits), in units of the
products they enter; for element-wise gradients A = |ref|."""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

from tests import attn_cases, norm_cases
from tests.hip_util import abs_mm64
from tests.norm_cases import dgelu64, gelu64

BF = torch.bfloat16
U = 2.0 ** -8                  # a bf16 store of the gradient itself
TINY = attn_cases.TINY         # the absolute floor of the cases modules
# One constant per Function family, in units of the absolute twin A.  Each starts from the rounding the family performs inside the graph
# and was set on the first MI355X run to the smallest power of two variant (a) -- every input live -- needs over all entries of the
# family (the needed value and the gradient that needed it beside it; test_all_live prints them); it is not to be raised to admit
# another variant.
CONST = {
    # plain / bias / residual need nothing beyond the bf16 store of the result (fp32 accumulation, gemm_cases 2^-20).  With GELU dH is a
    # bf16 tensor and gelu' reads the bf16 pre-activation; an unfolded DropPath factor makes s * dY a bf16 tensor: 2^-9 per product
    "linear": 2.0 ** -9,       # needed 2^-9.50, linear-gelu-rs dx
    # H, gelu(H) and dH are bf16 tensors between the four GEMMs (2^-9 each, per product), s * dY too when DropPath is not folded
    "mlp": 2.0 ** -8,          # needed 2^-8.15, mlp64-rs-nofold dw2
    # as "mlp" for dW1 / db1 / dW2 / db2, with xhat a bf16 tensor as well ...
    "ln_mlp": 2.0 ** -8,       # needed 2^-8.31, lnmlp-rs-nofold dw2
    # ... while dx, dgamma = colsum(dW1' * W1) and dbeta = W1^T db1 sum those GEMM results once more: their twin sums magnitudes over
    # hidden units AND rows, which the roundings (independent, of both signs) stay far below.  Kept apart so that the looser need of the
    # weight gradients cannot hide a wrong dgamma / dbeta (tests/test_autograd_graphs_host.py plants one)
    "ln_mlp_ln": 2.0 ** -15,   # needed 2^-15.23, lnmlp-rs-nofold dx
    # fp32 row and column sums (norm_cases SUM / RED count per add; here per sum).  Not calibrated: no element of any LayerNorm entry needed
    # more than the bf16 store term
    "ln": 2.0 ** -20,
    # the logits are a bf16 tensor (p moves by 2^-9 (|x| + |lse|) p), dlogits a bf16 tensor, _LibLinear rounds db to bf16
    "lib": 2.0 ** -8,          # needed 2^-8.78, lib-seq-37x24 dw
    "win": 2.0 ** 0,           # multiplies the kernel-level bound of attn_cases (its own CONST per term): 1 = the ABI bound unchanged
    "mha": 2.0 ** 0,           # the same for _MHA / _MHAPacked; largest use 0.71 of it, mha-qkv-d64-causal
    "win_linear": 2.0 ** -9,   # the qkv projection under window attention: dqkv is a bf16 tensor; needed 2^-9.48, win-linear-s3 dx
    "packed": 2.0 ** -10,      # the fork adds the alias gradient in the dgrad epilogue, one rounding for both; needed 2^-10.82, packed-fork dx
    "ew": 2.0 ** -20,          # fp32 element-wise math and dots (ew_cases EW / SUM); not calibrated: nothing needed beyond the bf16 store
    "embed": 2.0 ** -20,       # the embedding LayerNorm's fp32 sums (ew_cases EMB counts per term; here per sum); not calibrated either
}


class Case:
    def __init__(self, leaves, params, extra, gs):
        self.leaves, self.params, self.extra, self.gs = OrderedDict(leaves), tuple(params), extra, list(gs)


class Entry:
    def __init__(self, name, family, make, run, ref, twin, leaf_family=None):
        self.name, self.family, self.make, self.run, self.ref, self.twin = name, family, make, run, ref, twin
        self.leaf_family = leaf_family or {}
        self._cases = {}

    def fam(self, leaf):
        """the constant a leaf's gradient is bounded with"""
        return self.leaf_family.get(leaf, self.family)

    def case(self, device):
        if str(device) not in self._cases:
            self._cases[str(device)] = self.make(device)
        return self._cases[str(device)]

    def __repr__(self):
        return self.name


class _Rnd(torch.autograd.Function):
    """A bf16 store in the host emulation: rounds the value forward (fwd) and the gradient backward (bwd)."""

    @staticmethod
    def forward(ctx, v, fwd, bwd):
        ctx.bwd = bwd
        return v.to(BF).to(v.dtype) if fwd else v.view_as(v)

    @staticmethod
    def backward(ctx, g):
        return (g.to(BF).to(g.dtype) if ctx.bwd else g), None, None


def rn_bf16(v, fwd=True, bwd=True):
    """fwd=False / bwd=False: the value / its gradient stays in fp32 registers inside a fused kernel"""
    return _Rnd.apply(v, fwd, bwd)


def rn_none(v, fwd=True, bwd=True):
    return v


def plain_mid(t, f):
    return f(t)


def _gen(name, device=None):
    """Inputs are drawn on the host and moved: the GPU tests and the host tests read the same values."""
    return torch.Generator().manual_seed(1 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100003)


def _randn(shape, g, device, std=1.0):
    return (torch.randn(*shape, generator=g) * std).to(device)


def _bf(shape, g, device, std=1.0):
    return (torch.randn(*shape, generator=g) * std).to(BF).to(device)


def _f32x(shape, g, device, std=1.0):
    """fp32 with bf16-exact values: what an fp32 master parameter's bf16 working copy holds"""
    return _bf(shape, g, device, std).float()


def d2gelu64(x):
    return torch.exp(-0.5 * x * x) * (2 * math.pi) ** -0.5 * (2.0 - x * x)


def gelu_twin(ds_abs, pre):
    """Absolute twin of dH = dS gelu'(pre): |dS| (|gelu'| + |pre gelu''| + 2^-4).  The kernels read the bf16 pre-activation (it moves
    by 2^-9 |pre|, gelu' by that times gelu'') and a polynomial gelu' with |error| <= 2^-12 = 2^-4 * 2^-8 (norm_cases.GELU_BWD_ERR)."""
    return ds_abs * (dgelu64(pre).abs() + (pre * d2gelu64(pre)).abs() + 2.0 ** -4)


def _rows(t):
    return t.reshape(-1, t.shape[-1])


def _rs_rows(rs, like):
    """per-sample factor as a column over the rows of `like` ([B, R, N] -> [B * R, 1])"""
    return rs.to(like.dtype).repeat_interleave(like.numel() // like.shape[-1] // rs.numel())[:, None]


def _payload(t, t32):
    """value of the fp32 payload, gradient to its bf16 shadow"""
    return t + (t32.to(t.dtype) - t.detach())


# ---- _Linear ------------------------------------------------------------------------------------------------------------------------
def _linear_entry(name, bias=False, act=False, res=False, rs=None, res32=False, R=64):
    B, K, N = 3, 64, 64

    def make(device):
        g = _gen(name, device)
        leaves = [("x", _bf((B, R, K), g, device)), ("w", _f32x((N, K), g, device, K ** -0.5))]
        if bias:
            leaves.append(("b", _f32x((N,), g, device, 0.1)))
        if res:
            leaves.append(("res", _bf((B, R, N), g, device)))
        E = {}
        if rs:
            E["rs"] = torch.tensor([1.25, 0.0, 1.25], device=device)
            E["rsv"] = 1.25
        if res32:
            E["res32"] = dict(leaves)["res"].float() + _randn((B, R, N), g, device, 2.0 ** -10)
        return Case(leaves, ["w"] + (["b"] if bias else []), E, [_bf((B, R, N), g, device)])

    def run(ops, L, E, mid=plain_mid):
        r = L.get("res")
        if "res32" in E:
            r = ops.with_f32(r, E["res32"])
        return (ops.linear(L["x"], L["w"], L.get("b"), residual=r, act=act, rowscale=E.get("rs"), rowscale_value=E.get("rsv")),)

    def ref(L, E, mid=plain_mid, rn=rn_none):
        pre = F.linear(L["x"], L["w"].to(L["x"].dtype), L["b"].to(L["x"].dtype) if bias else None)
        z = gelu64(rn(pre)) if act else pre
        if rs:
            z = z * E["rs"].to(z.dtype)[:, None, None]
        if res:
            z = z + (_payload(L["res"], E["res32"]) if res32 else L["res"])
        return (rn(z),)

    def twin(L, E, gs, dmid=None):
        x, w, dy = _rows(L["x"]).double(), L["w"].double(), _rows(gs[0]).double()
        ds = dy * _rs_rows(E["rs"], gs[0]).double() if rs else dy
        if act:
            pre = x @ w.t() + (L["b"].double() if bias else 0.0)
            dh = gelu_twin(ds.abs(), pre)
        else:
            dh = ds.abs()
        A = {"x": abs_mm64(dh, w.t()).view(L["x"].shape), "w": abs_mm64(dh.t(), x.t()), "b": dh.sum(0)}
        if res:
            A["res"] = gs[0].double().abs()
        return A

    return Entry(name, "linear", make, run, ref, twin)


# ---- _MLP ---------------------------------------------------------------------------------------------------------------------------
def _mlp_entry(name, C, rs=None, R=64):
    B = 3

    def make(device):
        g = _gen(name, device)
        leaves = [("x", _bf((B, R, C), g, device)), ("w1", _f32x((4 * C, C), g, device, C ** -0.5)), ("b1", _f32x((4 * C,), g, device, 0.1)),
                  ("w2", _f32x((C, 4 * C), g, device, (4 * C) ** -0.5)), ("b2", _f32x((C,), g, device, 0.1)), ("res", _bf((B, R, C), g, device))]
        E = {"rs": torch.tensor([1.25, 0.0, 1.25], device=device), "rsv": 1.25} if rs else {}
        return Case(leaves, ["w1", "b1", "w2", "b2"], E, [_bf((B, R, C), g, device)])

    def run(ops, L, E, mid=plain_mid):
        return (ops.mlp(L["x"], L["w1"], L["b1"], L["w2"], L["b2"], residual=L["res"], rowscale=E.get("rs"), rowscale_value=E.get("rsv")),)

    def ref(L, E, mid=plain_mid, rn=rn_none):
        dt = L["x"].dtype
        h = rn(F.linear(L["x"], L["w1"].to(dt), L["b1"].to(dt)))
        z = F.linear(rn(gelu64(h)), L["w2"].to(dt), L["b2"].to(dt))
        if rs:
            z = z * E["rs"].to(dt)[:, None, None]
        return (rn(z + L["res"]),)

    def twin(L, E, gs, dmid=None):
        x, w1, w2, dy = _rows(L["x"]).double(), L["w1"].double(), L["w2"].double(), _rows(gs[0]).double()
        dz = (dy * _rs_rows(E["rs"], gs[0]).double() if rs else dy).abs()
        h = x @ w1.t() + L["b1"].double()
        dh = gelu_twin(abs_mm64(dz, w2.t()), h)
        return {"x": abs_mm64(dh, w1.t()).view(L["x"].shape), "w1": abs_mm64(dh.t(), x.t()), "b1": dh.sum(0),
                "w2": abs_mm64(dz.t(), gelu64(h).t()), "b2": dz.sum(0), "res": gs[0].double().abs()}

    return Entry(name, "mlp", make, run, ref, twin)


# ---- _LayerNorm / _LayerNormRes -----------------------------------------------------------------------------------------------------
def _ln_entry(name, with_res, x32=False, y32=False, rows=77, C=96):
    eps = 1e-5

    def make(device):
        g = _gen(name, device)
        leaves = [("x", _bf((rows, C), g, device)), ("gamma", 1.0 + _f32x((C,), g, device, 0.25)), ("beta", _f32x((C,), g, device, 0.25))]
        E = {"x32": leaves[0][1].float() + _randn((rows, C), g, device, 2.0 ** -10)} if x32 else {}
        return Case(leaves, ["gamma", "beta"], E, [_bf((rows, C), g, device) for _ in range(2 if with_res else 1)])

    def run(ops, L, E, mid=plain_mid):
        x = ops.with_f32(L["x"], E["x32"]) if x32 else L["x"]
        if with_res:
            return tuple(ops.layernorm_res(x, L["gamma"], L["beta"], eps))
        y = ops.layernorm(x, L["gamma"], L["beta"], eps, want_f32=y32)
        assert (ops.f32_of(y) is not None) == y32               # the fp32 copy of the output: a second, non-differentiable output of the node
        return (y,)

    def ref(L, E, mid=plain_mid, rn=rn_none):
        dt = L["x"].dtype
        xv = _payload(L["x"], E["x32"]) if x32 else L["x"]
        y = rn(F.layer_norm(xv, (C,), L["gamma"].to(dt), L["beta"].to(dt), eps))
        return (y, L["x"].view_as(L["x"])) if with_res else (y,)

    def twin(L, E, gs, dmid=None):
        xv = (E["x32"] if x32 else L["x"]).double()
        out, _ = norm_cases.ln_fwd_reference(xv, L["gamma"], L["beta"], eps)
        dres = gs[1].double() if with_res and gs[1] is not None else None
        dy = gs[0].double() if gs[0] is not None else torch.zeros_like(xv)
        _, b = norm_cases.ln_bwd_reference(xv, dy, L["gamma"], out["mean"], out["rstd"], dres, None)
        n = norm_cases.red_depth(rows, C)
        A = {"x": b["dx"][1]["SUM"] + (dres.abs() if dres is not None else 0.0), "gamma": b["dgamma"][1]["RED"] / n, "beta": b["dbeta"][1]["RED"] / n}
        return A

    return Entry(name, "ln", make, run, ref, twin)


# ---- _LibLinear under _CrossEntropy / _SeqLogProb -----------------------------------------------------------------------------------
IGNORE, PAD = -100, 1


def _lib_entry(name, kind, rows, V, K=48):
    def make(device):
        g = _gen(name, device)
        lab = torch.randint(2, V, (rows,), generator=g)
        lab[torch.rand(rows, generator=g) < 0.8] = IGNORE if kind == "ce" else PAD
        lab[0] = 3
        lab = lab.to(device)
        leaves = [("h", _bf((rows, K), g, device)), ("w", _bf((V, K), g, device, 0.3)), ("b", _bf((V,), g, device, 0.1))]
        gs = [torch.tensor(0.75, device=device)] if kind == "ce" else [_randn((rows,), g, device)]
        return Case(leaves, ["w", "b"], {"lab": lab}, gs)

    def loss_of(ops, logits, lab):
        return ops.cross_entropy(logits, lab, IGNORE) if kind == "ce" else ops.seq_logprob(logits, lab, PAD)

    def run(ops, L, E, mid=plain_mid):
        return (mid(ops.lib_linear(L["h"], L["w"], L["b"]), lambda t: loss_of(ops, t, E["lab"])),)

    def ref_loss(t, lab):
        if kind == "ce":
            return F.cross_entropy(t, lab, ignore_index=IGNORE)
        lp = torch.log(torch.softmax(t, 1).gather(1, lab[:, None])[:, 0] + 1e-9)
        return torch.where(lab == PAD, torch.zeros_like(lp), lp)

    def ref(L, E, mid=plain_mid, rn=rn_none):
        return (mid(rn(F.linear(L["h"], L["w"], L["b"])), lambda t: ref_loss(t, E["lab"])),)

    def twin(L, E, gs, dmid=None):
        h, w, lab = L["h"].double(), L["w"].double(), E["lab"]
        x = h @ w.t() + L["b"].double()
        lse = torch.logsumexp(x, 1, keepdim=True)
        p = torch.exp(x - lse)
        valid = lab != (IGNORE if kind == "ce" else PAD)
        oh = torch.zeros_like(p)
        oh[torch.arange(rows, device=p.device), lab.clamp(0, V - 1)] = 1.0
        scale = (gs[0].double().abs() / valid.sum().clamp(min=1)).expand(rows) if kind == "ce" else gs[0].double().abs()
        # dlogits = (p - onehot) scale: p moves by p (|x| + |lse|) 2^-9 with the bf16 logits
        dl = (p * (1.0 + x.abs() + lse.abs()) + oh) * (scale * valid)[:, None]
        if dmid is not None:
            dl = dl + dmid.double().abs()
        return {"h": abs_mm64(dl, w.t()), "w": abs_mm64(dl.t(), h.t()), "b": dl.sum(0)}

    return Entry(name, "lib", make, run, ref, twin)


# ---- _Linear / _LinearQKVHeadMajor under _WindowAttn --------------------------------------------------------------------------------
def _win_entry(name, shift, head_major):
    Bn, H, W, heads, ws = 2, 14, 14, 2, 7
    C = heads * 32
    acase = attn_cases._win(name, Bn, H, W, heads, ws, shift, layout=1 if head_major else 0)

    def make(device):
        g = _gen(name, device)
        leaves = [("x", _bf((Bn, H * W, C), g, device)), ("w", _f32x((3 * C, C), g, device, C ** -0.5)), ("b", _f32x((3 * C,), g, device, 0.1)),
                  ("table", _randn(((2 * ws - 1) ** 2, heads), g, device, 0.5))]
        tok, lab, rel = attn_cases.window_geometry(Bn, H, W, ws, shift, device)
        E = dict(tok=tok, lab=lab, rel=rel, cols=attn_cases.qkv_columns(C, heads, acase["layout"], device))
        return Case(leaves, ["w", "b", "table"], E, [_bf((Bn, H * W, C), g, device)])

    def run(ops, L, E, mid=plain_mid):
        qkv = ops.linear_qkv_head_major(L["x"], L["w"], L["b"], heads) if head_major else ops.linear(L["x"], L["w"], L["b"])
        E["qkv_seen"] = qkv.detach()
        return (mid(qkv, lambda t: ops.window_attention(t, L["table"], Bn, H, W, heads, ws, shift, head_major=head_major)),)

    def grads(L, E, gs, dmid=None, qkv=None):
        """fp64 gradients and their twins of the two-Function graph, Function by Function: the window attention by
        attn_cases.window_reference on the bf16 qkv the kernel read (`qkv`; default: the fp64 projection rounded to bf16), the
        projection from that dqkv (+ dmid, the gradient of a second consumer of qkv)."""
        x, w = _rows(L["x"]).double(), L["w"].double()
        perm = E["cols"].reshape(-1)                                   # column of the qkv row that holds canonical channel (which, head, d)
        if qkv is None:
            qkv = torch.empty(x.shape[0], 3 * C, dtype=torch.float64, device=x.device)
            qkv[:, perm] = x @ w.t() + L["b"].double()
            qkv = qkv.to(BF)
        inp = dict(qkv=_rows(qkv), table=L["table"], do=_rows(gs[0]), cols=E["cols"], tok=E["tok"], lab=E["lab"], rel=E["rel"])
        r, t = attn_cases.window_reference(acase, inp)
        dq = torch.stack([r["dq"], r["dk"], r["dv"]], 1).reshape(-1, 3 * C)          # canonical [rows, 3, heads, 32]
        if dmid is not None:
            dq = dq + _rows(dmid).double()[:, perm]
        A = {"x": abs_mm64(dq, w.t()).view(L["x"].shape), "w": abs_mm64(dq.t(), x.t()), "b": dq.abs().sum(0)}
        G = {"x": (dq @ w).view(L["x"].shape), "w": dq.t() @ x, "b": dq.sum(0), "table": r["dtable"]}
        Bd = {k: bound("win_linear", G[k], A[k]) for k in A}
        Bd["table"] = CONST["win"] * (sum(attn_cases.CONST[c] * v for c, v in t["dtable"][1].items()) + t["dtable"][0])
        return G, Bd, A

    e = Entry(name, "win_linear", make, run, None, None)
    e.grads, e.acase = grads, acase
    return e


# ---- _LinearPacked ------------------------------------------------------------------------------------------------------------------
def _packed_entry(name, fork):
    B, Ln, C = 2, 40, 64

    def make(device):
        g = _gen(name, device)
        leaves = [("x", _bf((B, Ln, C), g, device))]
        for i in range(2):
            leaves += [(f"w{i}", _f32x((C, C), g, device, C ** -0.5)), (f"b{i}", _f32x((C,), g, device, 0.1))]
        gs = [_bf((B, Ln, 2 * C), g, device)] + ([_bf((B, Ln, C), g, device)] if fork else [])
        return Case(leaves, ["w0", "b0", "w1", "b1"], {}, gs)

    def run(ops, L, E, mid=plain_mid):
        sink = [] if fork else None
        y = ops.linear_packed(L["x"], [(L["w0"], L["b0"]), (L["w1"], L["b1"])], fork_sink=sink)
        return (y, sink[0] if sink else None) if fork else (y,)

    def ref(L, E, mid=plain_mid, rn=rn_none):
        dt = L["x"].dtype
        y = rn(torch.cat([F.linear(L["x"], L[f"w{i}"].to(dt), L[f"b{i}"].to(dt)) for i in range(2)], -1))
        return (y, L["x"].view_as(L["x"]) if L["x"].requires_grad else None) if fork else (y,)

    def twin(L, E, gs, dmid=None):
        x = _rows(L["x"]).double()
        dy = _rows(gs[0]).double() if gs[0] is not None else torch.zeros(x.shape[0], 2 * C, dtype=torch.float64, device=x.device)
        wc = torch.cat([L["w0"], L["w1"]]).double()
        A = {"x": abs_mm64(dy, wc.t()).view(L["x"].shape)}
        if fork and gs[1] is not None:
            A["x"] = A["x"] + gs[1].double().abs()
        for i in range(2):
            A[f"w{i}"], A[f"b{i}"] = abs_mm64(dy[:, i * C:(i + 1) * C].t(), x.t()), dy[:, i * C:(i + 1) * C].abs().sum(0)
        return A

    return Entry(name, "packed", make, run, ref, twin)


# ---- _ScaleAdd / _Add / _StreamAdd / _RowScaleAdd -----------------------------------------------------------------------------------
def _ew_entry(name, op, b=True, alpha=True, rs=False, res=True, res32=False):
    B, R, C = 3, 40, 64

    def make(device):
        g = _gen(name, device)
        leaves = [("a", _bf((B, R, C), g, device))]
        if b:
            leaves.append(("b", _bf((B, R, C), g, device)))
        if alpha:
            leaves.append(("alpha", torch.tensor([0.375], device=device)))
        if res:
            leaves.append(("res", _bf((B, R, C), g, device)))
        E = {"rs": torch.tensor([1.25, 0.0, 1.25], device=device)} if rs else {}
        if res32:
            E["res32"] = dict(leaves)["res"].float() + _randn((B, R, C), g, device, 2.0 ** -10)
        return Case(leaves, ["alpha"] if alpha else [], E, [_bf((B, R, C), g, device)])

    def run(ops, L, E, mid=plain_mid):
        if op == "scale_add":
            return (ops.scale_add(L["a"], L["b"], L["alpha"]),)
        if op == "add":
            return (ops.add(L["a"], L["b"]),)
        if op == "rowscale_add":
            return (ops.rowscale_add(L["res"], L["a"], E["rs"]),)
        r = L.get("res")
        if res32:
            r = ops.with_f32(r, E["res32"])
        return (ops.stream_add(r, L["a"], L.get("b"), L.get("alpha"), E.get("rs")),)

    def ref(L, E, mid=plain_mid, rn=rn_none):
        dt = L["a"].dtype
        v = L["a"]
        if b:
            v = v + (L["alpha"].to(dt) * L["b"] if alpha else L["b"])
        if rs:
            v = v * E["rs"].to(dt)[:, None, None]
        if res:
            v = v + (_payload(L["res"], E["res32"]) if res32 else L["res"])
        return (rn(v),)

    def twin(L, E, gs, dmid=None):
        dy = gs[0].double()
        ds = dy * E["rs"].double()[:, None, None] if rs else dy
        A = {"a": ds.abs(), "res": dy.abs()}
        if b:
            A["b"] = ds.abs() * (L["alpha"].double().abs() if alpha else 1.0)
        if alpha:
            A["alpha"] = (ds * L["b"].double()).abs().sum().reshape(1)
        return A

    return Entry(name, "ew", make, run, ref, twin)


# ---- _LnMlp -------------------------------------------------------------------------------------------------------------------------
def _ln_mlp_entry(name, rs=None):
    B, R, C, eps = 2, 64, 128, 1e-5

    def make(device):
        g = _gen(name, device)
        # gamma is a power of two per channel: the kernels read W1' = bf16(W1 diag(gamma)), which then holds exactly the reference's product
        gamma = (2.0 ** torch.randint(-1, 2, (C,), generator=g).float()).to(device)
        leaves = [("x", _bf((B, R, C), g, device)), ("gamma", gamma), ("beta", _f32x((C,), g, device, 0.25)),
                  ("w1", _f32x((4 * C, C), g, device, C ** -0.5)), ("b1", _f32x((4 * C,), g, device, 0.1)),
                  ("w2", _f32x((C, 4 * C), g, device, (4 * C) ** -0.5)), ("b2", _f32x((C,), g, device, 0.1))]
        E = {"rs": torch.tensor([1.25, 0.0], device=device)} if rs else {}
        if rs == "fold":                                        # 1 / keep known to the caller: the factor rides in the weight-gradient kernel
            E["rsv"] = 1.25
        return Case(leaves, ["gamma", "beta", "w1", "b1", "w2", "b2"], E, [_bf((B, R, C), g, device)])

    def run(ops, L, E, mid=plain_mid):
        assert ops.ln_mlp_eligible(L["x"], C)
        return (ops.ln_mlp(L["x"], L["gamma"], L["beta"], eps, L["w1"], L["b1"], L["w2"], L["b2"], E.get("rs"), E.get("rsv")),)

    def ref(L, E, mid=plain_mid, rn=rn_none):
        dt = L["x"].dtype
        # the fused kernels keep dxn, H and dG in registers: bf16 are xhat, gelu(H) (the weight-gradient GEMMs' operands) and dH
        xn = rn(F.layer_norm(L["x"], (C,), L["gamma"].to(dt), L["beta"].to(dt), eps), bwd=False)
        h = rn(F.linear(xn, L["w1"].to(dt), L["b1"].to(dt)), fwd=False)
        z = F.linear(rn(gelu64(h), bwd=False), L["w2"].to(dt), L["b2"].to(dt))
        if rs:
            z = z * E["rs"].to(dt)[:, None, None]
        return (rn(L["x"] + z),)

    def twin(L, E, gs, dmid=None):
        x, w1, w2, dy = _rows(L["x"]).double(), L["w1"].double(), L["w2"].double(), _rows(gs[0]).double()
        out, _ = norm_cases.ln_fwd_reference(x, L["gamma"], L["beta"], eps)
        xn = out["y"]
        dz = (dy * _rs_rows(E["rs"], gs[0]).double() if rs else dy).abs()
        h = xn @ w1.t() + L["b1"].double()
        dh = gelu_twin(abs_mm64(dz, w2.t()), h)
        dxn = abs_mm64(dh, w1.t())
        _, b = norm_cases.ln_bwd_reference(x, dxn, L["gamma"], out["mean"], out["rstd"], None, None)
        return {"x": (b["dx"][1]["SUM"] + dy.abs()).view(L["x"].shape), "gamma": (dxn * out["xhat"].abs()).sum(0), "beta": dxn.sum(0),
                "w1": abs_mm64(dh.t(), xn.t()), "b1": dh.sum(0), "w2": abs_mm64(dz.t(), gelu64(h).t()), "b2": dz.sum(0)}

    return Entry(name, "ln_mlp", make, run, ref, twin, leaf_family={k: "ln_mlp_ln" for k in ("x", "gamma", "beta")})


# ---- _PatchMergeLN ------------------------------------------------------------------------------------------------------------------
def _patch_merge_entry(name, x32=False):
    B, H, W, C, eps = 2, 8, 8, 32, 1e-5

    def make(device):
        g = _gen(name, device)
        leaves = [("x", _bf((B, H * W, C), g, device)), ("gamma", 1.0 + _f32x((4 * C,), g, device, 0.25)), ("beta", _f32x((4 * C,), g, device, 0.25))]
        E = {"x32": leaves[0][1].float() + _randn((B, H * W, C), g, device, 2.0 ** -10)} if x32 else {}
        return Case(leaves, ["gamma", "beta"], E, [_bf((B, H * W // 4, 4 * C), g, device)])

    def run(ops, L, E, mid=plain_mid):
        return (ops.patch_merge_ln(ops.with_f32(L["x"], E["x32"]) if x32 else L["x"], L["gamma"], L["beta"], H, W, eps),)

    def ref(L, E, mid=plain_mid, rn=rn_none):
        dt = L["x"].dtype
        xv = _payload(L["x"], E["x32"]) if x32 else L["x"]
        y = F.layer_norm(norm_cases.merge_gather(xv, B, H, W, C), (4 * C,), L["gamma"].to(dt), L["beta"].to(dt), eps)
        return (rn(y).view(B, H * W // 4, 4 * C),)

    def twin(L, E, gs, dmid=None):
        rows = norm_cases.merge_gather((E["x32"] if x32 else L["x"]).double(), B, H, W, C)
        out, _ = norm_cases.ln_fwd_reference(rows, L["gamma"], L["beta"], eps)
        _, b = norm_cases.ln_bwd_reference(rows, _rows(gs[0]).double(), L["gamma"], out["mean"], out["rstd"], None, None)
        n = norm_cases.red_depth(rows.shape[0], 4 * C)
        return {"x": norm_cases.merge_scatter(b["dx"][1]["SUM"], B, H, W, C).view(L["x"].shape), "gamma": b["dgamma"][1]["RED"] / n,
                "beta": b["dbeta"][1]["RED"] / n}

    return Entry(name, "ln", make, run, ref, twin)


# ---- _MHA / _MHAPacked --------------------------------------------------------------------------------------------------------------
def _mha_entry(name, mode, B, heads, Lq, Lk, D, causal=False):
    """mode "sep": ops.mha on q, k, v; 0: mha_qkv_packed on [q | k | v]; 1: mha_kv_packed on q and [k | v].  The reference is
    attn_cases.mha_reference (fp64, with the kernel-level bound terms), so this entry has `grads` instead of ref / twin."""
    C = heads * D
    acase = attn_cases._mha(name, B, heads, Lq, Lk, D, [], [], mask="pad", causal=causal, pad=0)

    def make(device):
        g = _gen(name, device)
        q, k, v = _bf((B * Lq, C), g, device), _bf((B * Lk, C), g, device), _bf((B * Lk, C), g, device)
        if mode == "sep":
            leaves = [("q", q), ("k", k), ("v", v)]
        else:
            leaves = [("qkv", torch.cat([q, k, v], 1))] if mode == 0 else [("q", q), ("kv", torch.cat([k, v], 1))]
        km = torch.zeros(B, Lk, device=device)
        km[1, Lk - Lk // 3:] = -10000.0
        return Case(leaves, [], {"kmask": km}, [_bf((B * Lq, C), g, device)])

    def run(ops, L, E, mid=plain_mid):
        if mode == "sep":
            return (ops.mha(L["q"], L["k"], L["v"], E["kmask"], B, heads, D ** -0.5),)
        if mode == 0:
            return (ops.mha_qkv_packed(L["qkv"], E["kmask"], B, heads, D ** -0.5, causal=causal),)
        return (ops.mha_kv_packed(L["q"], L["kv"], E["kmask"], B, heads, D ** -0.5),)

    def grads(L, E, gs, dmid=None, qkv=None):
        if mode == "sep":
            q, k, v = L["q"], L["k"], L["v"]
        elif mode == 0:
            q, k, v = L["qkv"][:, :C], L["qkv"][:, C:2 * C], L["qkv"][:, 2 * C:]
        else:
            q, k, v = L["q"], L["kv"][:, :C], L["kv"][:, C:]
        out, terms = attn_cases.mha_reference(acase, dict(q=q, k=k, v=v, do=gs[0], kmask=E["kmask"], scale=D ** -0.5))
        flat = lambda t: t.permute(0, 2, 1, 3).reshape(-1, C)
        G = {n: flat(out[key]) for n, key in (("q", "dQ"), ("k", "dK"), ("v", "dV"))}
        Bd = {n: CONST["mha"] * flat(sum(attn_cases.CONST[c] * t for c, t in terms[key][1].items()) + terms[key][0])
              for n, key in (("q", "dQ"), ("k", "dK"), ("v", "dV"))}
        if mode == 0:
            G, Bd = {"qkv": torch.cat([G["q"], G["k"], G["v"]], 1)}, {"qkv": torch.cat([Bd["q"], Bd["k"], Bd["v"]], 1)}
        elif mode == 1:
            G, Bd = {"q": G["q"], "kv": torch.cat([G["k"], G["v"]], 1)}, {"q": Bd["q"], "kv": torch.cat([Bd["k"], Bd["v"]], 1)}
        return G, Bd, {}

    e = Entry(name, "mha", make, run, None, None)
    e.grads, e.acase = grads, acase
    return e


# ---- _Dropout -----------------------------------------------------------------------------------------------------------------------
def _dropout_entry(name, p=0.25, seed=1234):
    shape = (3, 40, 64)

    def make(device):
        g = _gen(name, device)
        E = {}
        if torch.device(device).type == "cuda":                 # the keep mask is the kernel's own: recovered from an all-ones input
            from fiber_amd import ops
            E["keep"] = ops._Dropout.apply(torch.ones(shape, dtype=BF, device=device), p, seed) != 0
        return Case([("x", _bf(shape, g, device))], [], E, [_bf(shape, g, device)])

    def run(ops, L, E, mid=plain_mid):
        return (ops._Dropout.apply(L["x"], p, seed),)

    def ref(L, E, mid=plain_mid, rn=rn_none):
        return (rn(L["x"] * E["keep"].to(L["x"].dtype) / (1.0 - p)),)

    def twin(L, E, gs, dmid=None):
        return {"x": gs[0].double().abs() * E["keep"].double() / (1.0 - p)}

    e = Entry(name, "ew", make, run, ref, twin)
    e.gpu_only = True
    return e


# ---- _PatchEmbedProj / _RobertaEmbed: parameters only, their first input never needs a gradient -------------------------------------
def _patch_embed_entry(name):
    B, H, W, C = 2, 32, 32, 64

    def make(device):
        g = _gen(name, device)
        E = {"img": _bf((B, 3, H, W), g, device).float()}       # the im2col kernel rounds the image to bf16
        return Case([("w", _f32x((C, 3, 4, 4), g, device, 48 ** -0.5)), ("b", _f32x((C,), g, device, 0.1))], ["w", "b"], E,
                    [_bf((B, H * W // 16, C), g, device)])

    def run(ops, L, E, mid=plain_mid):
        return (ops.patch_embed_proj(E["img"], L["w"], L["b"]),)

    def ref(L, E, mid=plain_mid, rn=rn_none):
        dt = L["w"].dtype
        return (rn(F.conv2d(E["img"].to(dt), L["w"], L["b"], stride=4).flatten(2).transpose(1, 2)),)

    def twin(L, E, gs, dmid=None):
        w0 = torch.zeros_like(L["w"], dtype=torch.float64).requires_grad_(True)
        with torch.enable_grad():
            y = F.conv2d(E["img"].double().abs(), w0, None, stride=4).flatten(2).transpose(1, 2)
            (aw,) = torch.autograd.grad(y, w0, gs[0].double().abs())
        return {"w": aw, "b": _rows(gs[0]).double().abs().sum(0)}

    return Entry(name, "linear", make, run, ref, twin)


def _roberta_embed_entry(name):
    from tests import ew_cases
    B, S, C, Vw, P, pad, eps = 2, 24, 64, 50, 40, 1, 1e-5

    def make(device):
        g = _gen(name, device)
        ids = torch.randint(2, Vw, (B, S), generator=g)
        ids[1, S - 7:] = pad
        leaves = [("word", _randn((Vw, C), g, device)), ("pos_tab", _randn((P, C), g, device)), ("type_tab", _randn((2, C), g, device)),
                  ("gamma", 1.0 + _randn((C,), g, device, 0.25)), ("beta", _randn((C,), g, device, 0.25))]
        return Case(leaves, [n for n, _ in leaves], {"ids": ids.to(device)}, [_bf((B, S, C), g, device)])

    def run(ops, L, E, mid=plain_mid):
        return (ops.roberta_embed(E["ids"], L["word"], L["pos_tab"], L["type_tab"], L["gamma"], L["beta"], pad, eps),)

    def ref(L, E, mid=plain_mid, rn=rn_none):
        ids = E["ids"]
        x = (F.embedding(ids, L["word"], padding_idx=pad) + F.embedding(ew_cases.roberta_positions(ids, pad), L["pos_tab"], padding_idx=pad)
             + L["type_tab"][0])
        return (rn(F.layer_norm(x, (C,), L["gamma"], L["beta"], eps)),)

    def twin(L, E, gs, dmid=None):
        ids = E["ids"]
        f = ew_cases.embed_fwd_ref(ids, L["word"], L["pos_tab"], L["type_tab"], L["gamma"], L["beta"], pad, eps)
        r = ew_cases.embed_bwd_ref(ids, f["pos"], gs[0], L["gamma"], f["x"], f["mean"], f["rstd"], Vw, P, pad)
        tt = torch.zeros(2, C, dtype=torch.float64, device=ids.device)
        tt[0] = r["dtype"][1]
        return {"word": r["dword"][1], "pos_tab": r["dpos"][1], "type_tab": tt, "gamma": r["dgamma"][1], "beta": r["dbeta"][1]}

    return Entry(name, "embed", make, run, ref, twin)


ENTRIES = [
    _linear_entry("linear-plain"), _linear_entry("linear-bias", bias=True), _linear_entry("linear-gelu", bias=True, act=True),
    _linear_entry("linear-res", bias=True, res=True),
    _linear_entry("linear-rs-fold", bias=True, res=True, rs="fold"),                   # 64 rows per sample: DropPath rides in dgrad / wgrad
    _linear_entry("linear-rs-nofold", bias=True, res=True, rs="nofold", R=36),         # 36 rows per sample: a pass of its own
    _linear_entry("linear-gelu-rs", bias=True, act=True, rs="nofold"),                 # GELU is never folded
    _linear_entry("linear-res32", bias=True, res=True, res32=True),
    _mlp_entry("mlp64", 64), _mlp_entry("mlp64-rs-fold", 64, rs="fold"), _mlp_entry("mlp64-rs-nofold", 64, rs="nofold", R=36),
    _mlp_entry("mlp96", 96), _mlp_entry("mlp96-rs", 96, rs="nofold"),                  # C % 64 != 0: dgrad + gelu_bwd_colsum, never folded
    _ln_mlp_entry("lnmlp"), _ln_mlp_entry("lnmlp-rs", rs="fold"), _ln_mlp_entry("lnmlp-rs-nofold", rs="nofold"),
    _ln_entry("ln", False), _ln_entry("ln-x32", False, x32=True), _ln_entry("ln-y32", False, y32=True), _ln_entry("ln-x32-y32", False, x32=True, y32=True), _ln_entry("lnres", True), _ln_entry("lnres-x32", True, x32=True),
    _patch_merge_entry("patchmerge"), _patch_merge_entry("patchmerge-x32", x32=True),
    _lib_entry("lib-ce-37x24", "ce", 37, 24), _lib_entry("lib-ce-600x1000", "ce", 600, 1000),
    _lib_entry("lib-seq-37x24", "seq", 37, 24), _lib_entry("lib-seq-600x1000", "seq", 600, 1000),
    _win_entry("win-linear-s0", 0, False), _win_entry("win-linear-s3", 3, False),
    _win_entry("win-hm-s0", 0, True), _win_entry("win-hm-s3", 3, True),
    _packed_entry("packed", False), _packed_entry("packed-fork", True),
    _mha_entry("mha-sep-d64", "sep", 2, 2, 40, 40, 64), _mha_entry("mha-qkv-d64", 0, 2, 2, 40, 40, 64),
    _mha_entry("mha-qkv-d64-causal", 0, 2, 2, 40, 40, 64, causal=True), _mha_entry("mha-kv-d32", 1, 2, 4, 64, 40, 32),
    _dropout_entry("dropout"), _patch_embed_entry("patch-embed"), _roberta_embed_entry("roberta-embed"),
    _ew_entry("scale_add", "scale_add", res=False), _ew_entry("add", "add", alpha=False, res=False),
    _ew_entry("rowscale_add", "rowscale_add", b=False, alpha=False, rs=True),
    _ew_entry("stream-a", "stream", b=False, alpha=False), _ew_entry("stream-ab", "stream", alpha=False),
    _ew_entry("stream-ab-alpha", "stream"), _ew_entry("stream-ab-alpha-rs", "stream", rs=True),
    _ew_entry("stream-nores", "stream", res=False), _ew_entry("stream-res32", "stream", rs=True, res32=True),
]
BY_NAME = {e.name: e for e in ENTRIES}
assert len(BY_NAME) == len(ENTRIES)
AUTOGRAD = [e for e in ENTRIES if e.ref is not None]                 # entries whose reference is fp64 autograd of the plain operation
MANUAL = [e for e in ENTRIES if e.ref is None]                       # ... is the fp64 reference of attn_cases, Function by Function
HOST = [e for e in AUTOGRAD if not getattr(e, "gpu_only", False)]


# ---- running an entry ---------------------------------------------------------------------------------------------------------------
def leaves_of(case, live, dtype=None):
    """fresh leaves with requires_grad on the names in `live`; dtype: cast floating leaves (the fp64 / fp32 reference)"""
    out = OrderedDict()
    for k, v in case.leaves.items():
        t = v.detach().clone() if dtype is None else v.detach().to(dtype)
        out[k] = t.requires_grad_(k in live)
    return out


def backward(outs, gs, dtype=None):
    pairs = [(y, g if dtype is None else g.to(dtype)) for y, g in zip(outs, gs) if y is not None and g is not None and y.requires_grad]
    if pairs:
        torch.autograd.backward([p[0] for p in pairs], [p[1] for p in pairs])


def reference(entry, case, live, gs, mid=plain_mid, dmid=None):
    """({leaf: fp64 gradient or None}, {leaf: bound}) of an autograd entry with the leaves in `live` requiring a gradient"""
    L = leaves_of(case, live, torch.float64)
    outs = entry.ref(L, case.extra, mid)
    backward(outs, gs, torch.float64)
    with torch.no_grad():
        A = entry.twin({k: v.detach() for k, v in L.items()}, case.extra, gs, dmid)
    G = {k: L[k].grad for k in L}
    return G, {k: bound(entry.fam(k), G[k], A[k]) for k in L if G[k] is not None}, A


def bound(family, ref, A):
    return U * ref.abs() + CONST[family] * A + TINY


def needed(got, ref, A):
    """the constant this gradient needs: max over elements of (|got - ref| - 2^-8 |ref| - TINY) / A"""
    err = (got.double() - ref).abs() - U * ref.abs() - TINY
    return float((err / A.clamp_min(1e-300)).max().clamp_min(0.0))


def subsets(case):
    """(b): every single leaf frozen, every single leaf the only live one, parameters frozen, activations frozen"""
    names = list(case.leaves)
    acts = [n for n in names if n not in case.params]
    out = []
    for s in ([tuple(m for m in names if m != n) for n in names] + [(n,) for n in names] + [tuple(acts), tuple(case.params)]):
        if s and s not in out and len(s) < len(names):
            out.append(s)
    return out
