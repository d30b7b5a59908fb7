"""Autograd wrappers around the fiber_hip C ABI (fiber_amd/lib.py).

Activations are bf16, parameters stay fp32 masters (state-dict compatible with the reference); each op casts the
weights it needs to bf16 once per parameter version.  Forward GEMMs with fused epilogues, LayerNorm, all attention
cores, embeddings and the element-wise glue are hand-written HIP kernels, and so are both backward GEMMs of every linear:
dX = dY.W on the NT kernel (transposed bf16 working copy of W), dW = dY^T.X (+ the bias gradient) on the TN kernel
(csrc/gemm_tn.hip).  Only the caller-side heads (vocabulary decoder, 2-way ITM, VQA classifier) use the library GEMM.
The kernels need tensors on a HIP device; the detection, retrieval and decode ops also have host paths, and the accessors of the
derived weight copies are plain torch.

The derived weight copies (`_wcache`, `_packs`) follow their fp32 masters through a stamp, `_stamp(w)` = (version counter,
generation, storage address).  What changes one of the three is seen by itself: an in-place op on the parameter (`copy_`, `mul_`,
`load_state_dict`, torch's optimizers), `mark_weights_dirty()`, and `p.data = other` (`module.to()`, `module.float()`,
`vector_to_parameters`).  An in-place write THROUGH `p.data` (`p.data.mul_(2)`) changes none of them and cannot be seen from the
parameter: whoever writes that way calls `mark_weights_dirty()` afterwards -- that call is the contract.  FiberAdamW writes
through raw pointers and keeps its side of it in step() (restamp_bf16_copies and the two one-launch refreshes).
"""
import math
import os
import threading
import weakref

import torch

from . import lib

BF16 = torch.bfloat16
# Derived copies of parameters (bf16 / transposed / permuted working copies), keyed by (kind, id(parameter)).  The parameter
# itself is held WEAKLY: when a module is deleted its entries go with it (a finalizer purges them), so the cache neither keeps
# dead models' weights alive nor hands a stale copy to a new tensor that happens to reuse the id.
_wcache = {}


def _cache_get(key, w):
    hit = _wcache.get(key)
    if hit is not None and hit[2]() is w:
        return hit
    return None


def _cache_put(key, stamp, value, w):
    _wcache[key] = (stamp, value, weakref.ref(w, lambda _r, k=key: _wcache.pop(k, None)))


_WIN_COLSUM = os.environ.get("FIBER_WIN_COLSUM", "0") == "1"     # dqkv column sums inside the window backward (see _WindowAttn.backward)


_gen = [0]


def mark_weights_dirty():
    """Invalidate every cached bf16 working copy.  Fused / foreach optimizers update parameters through TensorList
    kernels that do NOT bump `Tensor._version`, so the version counter alone would leave stale weights in use;
    fiber_utils.set_schedule registers this as an optimizer step post-hook."""
    _gen[0] += 1


def _stamp(w):
    """What a derived copy was made from: the version counter (in-place ops on the parameter), the generation
    (mark_weights_dirty) and the storage address (`w.data = other` keeps the version: model.to(), module.float())."""
    return (w._version, _gen[0], w.data_ptr())


def bf16_weight(w):
    """bf16 copy of an fp32 parameter, refreshed when the parameter changes (version counter or optimizer step)."""
    key = id(w)
    hit = _cache_get(key, w)
    if hit is not None and hit[0] == _stamp(w) and hit[1].device == w.device:
        return hit[1]
    if hit is not None and hit[1].shape == w.shape and hit[1].device == w.device:
        wb = hit[1]
        wb.copy_(w.detach())                             # same storage: views into packed buffers / optimizer tables stay valid
    else:
        wb = w.detach().to(BF16).contiguous()
    _cache_put(key, _stamp(w), wb, w)
    return wb


def bf16_weight_t(w):
    """bf16 TRANSPOSED copy of an fp32 [N, K] parameter -> [K, N] (the B operand of the dgrad GEMM dX = dY . W in the
    kernel's NT form), refreshed when the parameter's version counter changes.  Copies made here are remembered: after an
    optimizer step refresh_transposed_copies() rewrites all of them in one launch instead of one strided copy per weight."""
    key = ("T", id(w))
    hit = _cache_get(key, w)
    if hit is not None and hit[0] == _stamp(w) and hit[1].device == w.device:
        return hit[1]
    wb = bf16_weight(w)
    if hit is not None and hit[1].shape == (wb.shape[1], wb.shape[0]) and hit[1].device == wb.device:
        wt = hit[1]
        wt.copy_(wb.t())                                 # same storage: pointer tables built on it stay valid
    else:
        wt = wb.t().contiguous()
    _cache_put(key, _stamp(w), wt, w)
    return wt


_tables = {}                         # (kernel, device) -> (what the rows hold: pointers AND shapes, device table, tiles)


def _launch_rows(kernel, by_dev, resolve=None):
    """One launch of a multi-tensor `kernel` per device over by_dev[device] = [(the pointers of one table row, N, K)].  The device
    table is kept and rebuilt when anything its rows hold changed; only then resolve(pointers, device) -> pointers runs."""
    for dev, want in by_dev.items():
        want = tuple(want)
        tab = _tables.get((kernel, dev))
        if tab is None or tab[0] != want:
            rows, tile0 = [], 0
            for ptrs, N, K in want:
                tk = -(-K // 64)
                rows.append((resolve(ptrs, dev) if resolve else ptrs) + (N | (K << 32), tile0 | (tk << 32)))
                tile0 += -(-N // 64) * tk
            tab = _tables[(kernel, dev)] = (want, torch.tensor(rows, dtype=torch.int64).to(dev), tile0)
        with torch.cuda.device(dev):
            lib.call(kernel, lib.ptr(tab[1]), len(want), tab[2])


def refresh_transposed_copies():
    """Rewrite every cached transposed copy whose plain bf16 copy is current (i.e. was just rewritten by the fused optimizer) in
    ONE kernel launch and mark it current.  Called by FiberAdamW.step() after it restamped the plain copies."""
    if not _wcache:
        return
    by_dev, done = {}, []                                # done: (the `_wcache` key or the pack, its masters)
    for key, (stamp, wt, ref) in list(_wcache.items()):
        if not (isinstance(key, tuple) and key[0] == "T"):
            continue
        w = ref()
        if w is None or not wt.is_cuda:
            continue
        plain = _cache_get(id(w), w)
        if plain is None or plain[0] != _stamp(w) or plain[1].shape != (wt.shape[1], wt.shape[0]):
            continue                                     # plain copy stale or gone: the lazy path rebuilds both
        if (wt.shape[0] % 8) or (wt.shape[1] % 8):
            continue
        by_dev.setdefault(wt.device, []).append(((plain[1].data_ptr(), wt.data_ptr()), wt.shape[1], wt.shape[0]))
        done.append((key, (w,)))
    for pk in list(_packs.values()):                      # packed projections (linear_packed): ONE descriptor per pack
        ws, plain = [r() for r in pk["refs"]], pk["plain"]
        if any(w is None for w in ws) or not plain.is_cuda:
            continue
        hits = [_cache_get(id(w), w) for w in ws]
        if any(h is None or h[0] != _stamp(w) for h, w in zip(hits, ws)) or not _pack_views_ok(pk, ws):
            continue                                         # some member stale: the lazy path (_pack_get) refreshes
        by_dev.setdefault(plain.device, []).append(((plain.data_ptr(), pk["t"].data_ptr()), plain.shape[0], plain.shape[1]))
        done.append((pk, ws))
    _launch_rows("fiber_transpose_multi_bf16", by_dev)
    for target, ws in done:
        if isinstance(target, dict):
            target["t_stamp"] = tuple(_stamp(w) for w in ws)         # a pack: its transposed copy is current
        else:
            _wcache[target] = (_stamp(ws[0]),) + _wcache[target][1:]


def _hm_row(ptrs, dev):
    return ptrs[:1] + (_qkv_perm32(*ptrs[1], dev).data_ptr(),) + ptrs[2:]


def refresh_head_major_copies():
    """Rewrite every cached head-major qkv working copy (permuted bf16 weight, its transpose, permuted fp32 bias: _LinearQKVHeadMajor) from the
    fp32 parameters in ONE launch and mark it current.  Called by FiberAdamW.step() after the parameter update, like refresh_transposed_copies();
    copies the optimizer did not touch are rewritten too (same values)."""
    by_dev, done = {}, []
    for key, (stamp, val, ref) in list(_wcache.items()):
        if not (isinstance(key, tuple) and key[0] == "HM"):
            continue
        w = ref()
        b = val[3]() if len(val) > 3 else None              # (a bias Parameter that was REPLACED: the forward checks identity and rebuilds)
        if w is None or b is None or not val[0].is_cuda or w.dtype != torch.float32 or b.dtype != torch.float32 or not w.is_contiguous():
            continue
        if (w.shape[0] % 8) or (w.shape[1] % 8):
            continue
        # the second pointer is the row permutation's: it stands here as (K, heads) and becomes an address when the table is built
        by_dev.setdefault(w.device, []).append(((w.data_ptr(), (w.shape[1], val[4]), val[0].data_ptr(), val[2].data_ptr(), b.data_ptr(), val[1].data_ptr()),
                                                w.shape[0], w.shape[1]))
        done.append((key, (w, b)))
    _launch_rows("fiber_rowperm_cast_multi_bf16", by_dev, _hm_row)
    for key, (w, b) in done:
        _wcache[key] = ((_stamp(w), _stamp(b)),) + _wcache[key][1:]


def bf16_copy_if_cached(w):
    """The cached bf16 working copy of `w` (whatever its state), or None -- for the fused optimizer, which rewrites it."""
    hit = _cache_get(id(w), w)
    return hit[1] if hit is not None else None


def restamp_bf16_copies(params, bump=True):
    """After an optimizer step that rewrote the plain bf16 copies in place: every other derived cache entry (transposed /
    permuted copies) is invalidated (`bump`, once per step), the rewritten ones are marked current."""
    if bump:
        _gen[0] += 1
    for w in params:
        hit = _cache_get(id(w), w)
        if hit is not None:
            _wcache[id(w)] = (_stamp(w), hit[1], hit[2])


def cast_bf16(w):
    """Autograd-visible bf16 view of an fp32 parameter for library GEMMs (gradient flows back in fp32)."""
    return w.to(BF16)


def clear_weight_cache():
    _wcache.clear()
    _packs.clear()
    _tables.clear()


def _rows(x):
    return x.numel() // x.shape[-1]


def _c(t):
    """t as contiguous memory whose base the kernels' 16-byte vector accesses accept: a contiguous view at an offset that is not a
    multiple of 16 bytes is copied (the entry points refuse such a base with FIBER_EINVAL)."""
    if t.is_contiguous() and t.data_ptr() % 16 == 0:
        return t
    return t.clone(memory_format=torch.contiguous_format)


# ---- fp32 residual stream ---------------------------------------------------------------------------------------------------
# config["residual_dtype"] = "fp32" keeps the residual streams of both backbones (Swin: x = x + branch, reference
# swin_transformer.py:388-391; RoBERTa: the LayerNorm inputs a + h / dense + input and the LayerNorm outputs that become the next
# residual, roberta.py:485,417-423) in fp32 instead of rounding them to bf16 at every block.  A stream tensor then travels as a
# PAIR: the bf16 tensor autograd sees (the "shadow": what GEMMs read, what gradients -- bf16 -- flow along) carrying the fp32
# payload as the attribute `_f32`.  Ops that sit on the stream (layernorm_res / layernorm / patch_merge_ln read it; the proj / fc2 /
# dense epilogues and stream_add write it) use the payload when it is there and fall back to the bf16 tensor when it is not (a
# tensor that was cloned / sliced by a caller simply loses the extra precision).  Gradients stay bf16 either way.
_RESIDUAL_FP32 = [os.environ.get("FIBER_RESIDUAL_DTYPE", "bf16").lower() in ("fp32", "float32")]


def set_residual_dtype(dtype):
    """"fp32" / torch.float32: new residual streams start in fp32 (see above); "bf16": the round-1/2 behaviour."""
    _RESIDUAL_FP32[0] = dtype in ("fp32", "float32", torch.float32)


def residual_fp32():
    return _RESIDUAL_FP32[0]


def f32_of(t):
    """The fp32 payload of a stream tensor, or None."""
    return getattr(t, "_f32", None) if t is not None else None


def with_f32(t16, t32):
    if t32 is not None:
        t16._f32 = t32
    return t16


def start_stream(t16):
    """A bf16 tensor that begins a residual stream (PatchMerging output, text embeddings): in fp32 mode attach its fp32 copy."""
    if _RESIDUAL_FP32[0] and f32_of(t16) is None:
        t16._f32 = t16.detach().float()
    return t16


# the `act` argument of fiber_gemm_nt_bf16, as include/fiber_hip.h defines it
ACT_GELU, ACT_GELU_BWD = lib.DEFINES["FIBER_ACT_GELU"], lib.DEFINES["FIBER_ACT_GELU_BWD"]
ACT_OUT_F32, ACT_STREAM_F32 = lib.DEFINES["FIBER_ACT_OUT_F32"], lib.DEFINES["FIBER_ACT_STREAM_F32"]


def gemm_nt(x2, wb, bias=None, residual=None, act=0, want_pre=False, rowscale=None, rows_per_sample=0, aux=None,
            want_colsum=False, out_fp32=False, res32=None):
    """y = act(x2 @ wb^T + bias) + residual  on the HIP kernel.  x2 [M,K] bf16 (row stride may exceed K).
    out_fp32 (plain / bias only): the result is stored in fp32.
    res32 (fp32 [M, N], instead of `residual`): the fp32 residual-stream form -- returns (y16, y32): the sum in fp32 and its
    bf16 shadow."""
    M, K = x2.shape
    N = wb.shape[0]
    assert x2.dtype == BF16 and wb.dtype == BF16 and x2.stride(1) == 1 and wb.stride(1) == 1
    if res32 is not None:
        assert res32.dtype == torch.float32 and res32.stride(1) == 1 and not act and residual is None and not want_colsum and not out_fp32
        y16 = torch.empty((M, N), dtype=BF16, device=x2.device)
        y32 = torch.empty((M, N), dtype=torch.float32, device=x2.device)
        lib.call("fiber_gemm_nt_bf16", lib.ptr(x2), lib.ptr(wb), lib.ptr(bias), lib.ptr(res32), lib.ptr(y16), lib.ptr(y32),
                 lib.ptr(rowscale), rows_per_sample, None, 0, None, M, N, K, x2.stride(0), wb.stride(0), N, res32.stride(0),
                 ACT_STREAM_F32)
        return y16, y32
    y = torch.empty((M, N), dtype=torch.float32 if out_fp32 else BF16, device=x2.device)
    if out_fp32:
        assert not act and residual is None and not want_colsum
        act = ACT_OUT_F32
    pre = torch.empty((M, N), dtype=BF16, device=x2.device) if (want_pre and act) else None
    colpart = None
    if want_colsum:
        tiles = -(-M // lib.plain("fiber_gemm_row_tile", M, N, K))
        colpart = torch.empty((tiles, N), dtype=torch.float32, device=x2.device)
    lib.call("fiber_gemm_nt_bf16", lib.ptr(x2), lib.ptr(wb), lib.ptr(bias), lib.ptr(residual), lib.ptr(y), lib.ptr(pre),
             lib.ptr(rowscale), rows_per_sample, lib.ptr(aux), aux.stride(0) if aux is not None else 0, lib.ptr(colpart),
             M, N, K, x2.stride(0), wb.stride(0), N, residual.stride(0) if residual is not None else 0, act)
    if want_colsum:
        cs = torch.empty(N, dtype=torch.float32, device=x2.device)
        lib.call("fiber_fold_rows_f32", lib.ptr(colpart), lib.ptr(cs), colpart.shape[0], N)
        return y, cs
    return y, pre


def gelu_bwd_colsum(dg, h):
    """dh = dg * gelu'(h) and its column sums (bias gradient) in one pass."""
    M, N = dg.shape
    dh = torch.empty_like(dg)
    db = torch.empty(N, dtype=torch.float32, device=dg.device)
    slabs = lib.plain("fiber_colsum_slabs", M, N)
    ws = torch.empty(slabs * N, dtype=torch.float32, device=dg.device) if slabs > 1 else None
    lib.call("fiber_gelu_bwd_colsum_bf16", lib.ptr(dg), lib.ptr(h), lib.ptr(dh), lib.ptr(db), lib.ptr(ws), M, N)
    return dh, db


def rowscale_colsum(dy2, rowscale):
    """ds = per-sample scale * dy and its column sums (bias gradient) in one pass."""
    M, N = dy2.shape
    ds = torch.empty_like(dy2)
    db = torch.empty(N, dtype=torch.float32, device=dy2.device)
    slabs = lib.plain("fiber_colsum_slabs", M, N)
    ws = torch.empty(slabs * N, dtype=torch.float32, device=dy2.device) if slabs > 1 else None
    lib.call("fiber_rowscale_colsum_bf16", lib.ptr(dy2), lib.ptr(rowscale), lib.ptr(ds), lib.ptr(db), lib.ptr(ws), M, N,
             M // rowscale.numel())
    return ds, db


def colsum(x2):
    if x2.data_ptr() % 16 or x2.stride(1) != 1 or x2.stride(0) % 8:
        x2 = _c(x2)
    M, N = x2.shape
    out = torch.empty(N, dtype=torch.float32, device=x2.device)
    slabs = lib.plain("fiber_colsum_slabs", M, N)
    ws = torch.empty(slabs * N, dtype=torch.float32, device=x2.device) if slabs > 1 else None
    lib.call("fiber_colsum_bf16", lib.ptr(x2), lib.ptr(out), lib.ptr(ws), M, N, x2.stride(0))
    return out


# ---- library GEMMs are kept in ONE global order across HIP streams ------------------------------------------------
# hipBLASLt picks stream-K kernels for many of these shapes (…_SK3_… in the rocprof traces): persistent grids whose
# workgroups spin on each other's partial tiles and therefore assume they are all resident.  Two of them in flight on two
# streams (the fused branch runs the text stack on a second stream) can each hold half the CUs and wait for the other half
# forever -- observed as a 100 %-busy GPU with both streams parked behind a library GEMM.  Every library GEMM issued from
# this package therefore waits for the previous one, whichever stream it was issued on (one event wait, only when the stream
# changes); library GEMMs still overlap with every other kernel.
_lib_gemm_last = {"event": None, "stream": None}


class lib_gemm:
    def __enter__(self):
        self.capturing = torch.cuda.is_current_stream_capturing()
        if self.capturing:                                   # one stream by construction: nothing to order
            return self
        self.cur = torch.cuda.current_stream()
        last = _lib_gemm_last
        if last["event"] is not None and last["stream"] != self.cur.cuda_stream:
            self.cur.wait_event(last["event"])
        return self

    def __exit__(self, *exc):
        if self.capturing:
            return False
        ev = torch.cuda.Event()
        ev.record(self.cur)
        _lib_gemm_last["event"], _lib_gemm_last["stream"] = ev, self.cur.cuda_stream
        return False


def lib_matmul(a, b):
    with lib_gemm():
        return torch.matmul(a, b)


class _LibLinear(torch.autograd.Function):
    """y = x.W^T + b on the library GEMM (caller-side heads: vocabulary decoder, ITM / VQA classifiers), forward and both
    backward GEMMs inside the global library-GEMM order."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        with lib_gemm():
            return torch.nn.functional.linear(x, w, b)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy2, x2 = dy.reshape(-1, dy.shape[-1]), x.reshape(-1, x.shape[-1])
        dx = dw = db = None
        hint = _take_labelled_rows(dy2)                      # every backward empties the slot, with or without a bias to use it for
        with lib_gemm():
            if ctx.needs_input_grad[0]:
                dx = torch.matmul(dy2, w).view(x.shape)
            if ctx.needs_input_grad[1]:
                dw = torch.matmul(dy2.t(), x2)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            # (more rows than the labelled-row kernel's slab plan holds: the plain sum, asked before any launch)
            if hint is not None and dy2.is_cuda and dy2.dtype == BF16 and dy2.shape[0] <= lib.plain("fiber_colsum_labelled_max_rows"):
                lab, ignore = hint                           # dlogits of _CrossEntropy: its ignored rows are zero, only the labelled ones are read
                M, N = dy2.shape
                slabs = lib.plain("fiber_colsum_labelled_slabs", M)
                db32 = torch.empty(N, dtype=torch.float32, device=dy2.device)
                ws = torch.empty(slabs * N, dtype=torch.float32, device=dy2.device) if slabs > 1 else None
                lib.call("fiber_colsum_labelled_bf16", lib.ptr(dy2), lib.ptr(lab), lib.ptr(db32), lib.ptr(ws), M, N, ignore)
                db = db32.to(dy2.dtype)                      # (what dy2.sum(0) returns: fp32 accumulation, one rounding)
            else:
                db = dy2.sum(0)
        return dx, dw, db


# _CrossEntropy.backward -> the linear that produced the logits: "the rows of this gradient whose label is the ignore index are zero".
# The statement is about the bytes the producer wrote, so it holds for the gradient a consumer receives only if that is the producer's
# tensor UNCHANGED: same address and shape, and the version counter the tensor had at the offer.  Autograd's fan-in adds another
# consumer's gradient into the first one in place, and a caller may write into a leaf's .grad (which is the producer's tensor): both
# bump the counter (views share it), and the offer is void.  Like the column-sum slot below, an offer never outlives the backward
# pass it was made in, and every _LibLinear.backward empties the slot; a missed hand-over only costs the plain column sum.
_rows_tls = threading.local()


def _clear_labelled_rows():
    _rows_tls.slot = None


def _offer_labelled_rows(dx, labels, ignore):
    """Called from inside a backward()."""
    _rows_tls.slot = (dx.data_ptr(), tuple(dx.shape), dx._version, labels, ignore)
    torch.autograd.Variable._execution_engine.queue_callback(_clear_labelled_rows)


def _take_labelled_rows(t2d):
    h = getattr(_rows_tls, "slot", None)
    _rows_tls.slot = None
    if h is not None and t2d.is_contiguous() and h[0] == t2d.data_ptr() and h[1] == tuple(t2d.shape) and h[2] == t2d._version:
        return h[3], h[4]
    return None


class _CrossEntropy(torch.autograd.Function):
    """mean over the non-ignored rows of logsumexp(x) - x[label] for bf16 logits [rows, V] (F.cross_entropy semantics with
    ignore_index), forward and backward on csrc/loss.hip: no fp32 copy of the logits, no log-softmax tensor."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index):
        rows, V = logits.shape
        x = _c(logits)
        lab = labels.contiguous()
        loss = torch.empty(rows, dtype=torch.float32, device=x.device)
        lse = torch.empty_like(loss)
        pred = torch.empty(rows, dtype=torch.int32, device=x.device)
        lib.call("fiber_ce_fwd_bf16", lib.ptr(x), lib.ptr(lab), lib.ptr(loss), lib.ptr(lse), lib.ptr(pred), rows, V, int(ignore_index))
        # arg max of the labelled rows (-1 on the others), for the accuracy metric: handed over on the logits object (fiber_utils.Accuracy)
        logits._fiber_argmax = (pred, lab, int(ignore_index))
        nvalid = (lab != ignore_index).sum().clamp(min=1).float()
        ctx.save_for_backward(x, lab, lse, nvalid)
        ctx.ignore = int(ignore_index)
        return loss.sum() / nvalid

    @staticmethod
    def backward(ctx, g):
        x, lab, lse, nvalid = ctx.saved_tensors
        scale = (g.float() / nvalid).reshape(1).contiguous()
        dx = torch.empty_like(x)
        lib.call("fiber_ce_bwd_bf16", lib.ptr(x), lib.ptr(lab), lib.ptr(lse), lib.ptr(scale), lib.ptr(dx), x.shape[0], x.shape[1],
                 ctx.ignore)
        _offer_labelled_rows(dx, lab, ctx.ignore)
        return dx, None, None


def cross_entropy(logits, labels, ignore_index=-100):
    """F.cross_entropy(logits.float(), labels, ignore_index=...) for bf16 logits [rows, V] (mean over valid rows)."""
    assert logits.dtype == BF16 and logits.dim() == 2 and labels.dtype == torch.int64
    return _CrossEntropy.apply(logits, labels, ignore_index)


class _SeqLogProb(torch.autograd.Function):
    """lp[r] = log(softmax(x[r])[labels[r]] + 1e-9), 0 where labels[r] == pad_id (objectives.py:818-824), for bf16 logits [rows, V] on
    csrc/loss.hip: one read of the logits forward, one read and one bf16 write backward, the per-row upstream gradient read on the device."""

    @staticmethod
    def forward(ctx, logits, labels, pad_id):
        rows, V = logits.shape
        x = _c(logits)
        lab = labels.contiguous()
        lp = torch.empty(rows, dtype=torch.float32, device=x.device)
        lse = torch.empty_like(lp)
        lib.call("fiber_seqlogp_fwd_bf16", lib.ptr(x), lib.ptr(lab), lib.ptr(lp), lib.ptr(lse), rows, V, int(pad_id))
        ctx.save_for_backward(x, lab, lse)
        ctx.pad = int(pad_id)
        return lp

    @staticmethod
    def backward(ctx, g):
        x, lab, lse = ctx.saved_tensors
        rowscale = g.float().contiguous()
        dx = torch.empty_like(x)
        lib.call("fiber_seqlogp_bwd_bf16", lib.ptr(x), lib.ptr(lab), lib.ptr(lse), lib.ptr(rowscale), lib.ptr(dx), x.shape[0], x.shape[1], ctx.pad)
        _offer_labelled_rows(dx, lab, ctx.pad)               # pad rows are exact zeros: the decoder-bias column sum skips them
        return dx, None, None


def seq_logprob(logits, labels, pad_id):
    """log(softmax(logits)[labels] + 1e-9) per row, 0 on rows whose label is pad_id: fp32 [rows].  bf16 device logits run on the HIP kernels;
    CPU tensors on the same formulas in torch (host tests)."""
    assert logits.dim() == 2 and labels.dtype == torch.int64 and labels.shape == logits.shape[:1]
    if not logits.is_cuda:
        x = logits.float()
        pad = labels == pad_id
        lab = labels.clamp(0, x.shape[1] - 1)
        p = torch.exp(x.gather(1, lab[:, None])[:, 0] - torch.logsumexp(x, 1))
        return torch.where(pad, torch.zeros_like(p), torch.log(p + 1e-9))
    assert logits.dtype == BF16
    return _SeqLogProb.apply(logits, labels, pad_id)


def _hash_u32_torch(key, idx):
    """hash_u32 of csrc/common.h on int64 tensors (two's-complement products are the uint64 ones; the shifts are made logical)."""
    def i64(v):
        v &= _M64
        return v - (1 << 64) if v >= (1 << 63) else v

    def shr(z, n):
        return (z >> n) & ((1 << (64 - n)) - 1)
    z = idx * i64(0x9E3779B97F4A7C15) + i64(int(key))
    z = (z ^ shr(z, 30)) * i64(0xBF58476D1CE4E5B9)
    z = (z ^ shr(z, 27)) * i64(0x94D049BB133111EB)
    z = z ^ shr(z, 31)
    return shr(z, 32)


SAMPLE_FORCED_LOGIT = -10000.0


def sample_rows(logits, K, forced_id, key=None, ended=None, pad_id=1, sep_id=2):
    """K tokens per row of `logits` [rows, V] drawn with replacement from softmax(logits) (column forced_id read as -10000) by Gumbel-max
    on a counter-based key: (tokens int64 [rows, K], logp fp32 [rows, K] = z_tok - logsumexp(z), ended uint8 [rows, K] = tok in {pad, sep}).
    Replaces log_softmax / exp_ / torch.multinomial(replacement=True) / gather of objectives.py:756-766, 781-786.  Rows with ended[r] != 0
    give pad_id / 0 / 1.  key=None draws a fresh key from the dropout key stream.  CPU tensors run the same formulas in torch (fp64)."""
    assert logits.dim() == 2
    rows, V = logits.shape
    if key is None:
        key = next_seed()
    if ended is not None:
        ended = ended.reshape(rows).to(torch.uint8).contiguous()
    if not logits.is_cuda:
        z = logits.double().clone()
        if forced_id >= 0:
            z[:, forced_id] = SAMPLE_FORCED_LOGIT
        idx = ((torch.arange(rows)[:, None, None] * K + torch.arange(K)[None, :, None]) * V + torch.arange(V)[None, None, :])
        u = (_hash_u32_torch(key, idx).double() + 0.5) * 2.0 ** -32
        tokens = (z[:, None, :] - torch.log(-torch.log(u))).argmax(-1)
        logp = (z.gather(1, tokens) - torch.logsumexp(z, 1, keepdim=True)).float()
        if ended is not None:
            e = ended.bool()[:, None]
            tokens = torch.where(e, torch.full_like(tokens, pad_id), tokens)
            logp = torch.where(e, torch.zeros_like(logp), logp)
        return tokens, logp, ((tokens == pad_id) | (tokens == sep_id)).to(torch.uint8)
    assert logits.dtype == BF16
    x = _c(logits)
    tokens = torch.empty(rows, K, dtype=torch.int64, device=x.device)
    logp = torch.empty(rows, K, dtype=torch.float32, device=x.device)
    ended_out = torch.empty(rows, K, dtype=torch.uint8, device=x.device)
    lib.call("fiber_sample_rows_bf16", lib.ptr(x), lib.ptr(ended), lib.ptr(tokens), lib.ptr(logp), lib.ptr(ended_out), rows, V, int(K),
             int(forced_id), int(key) & _M64, seed_base_ptr(), int(pad_id), int(sep_id))
    return tokens, logp, ended_out


# Call sites of the library GEMM (file names), recorded when a test switches it on: the library is allowed for the caller-side heads
#  and the ITC similarity matrices only -- tests/test_hip_modules.py::test_library_gemm_only_from_heads.
lib_gemm_sites = None


def _note_lib_site(depth=2):
    if lib_gemm_sites is not None:
        import sys
        f = sys._getframe(depth)
        lib_gemm_sites[os.path.basename(f.f_code.co_filename) + ":" + f.f_code.co_name] = lib_gemm_sites.get(
            os.path.basename(f.f_code.co_filename) + ":" + f.f_code.co_name, 0) + 1


def lib_linear(x, w, b=None):
    _note_lib_site()
    return _LibLinear.apply(x, w, b)


# Retired entry points.  bench.py calls set_fold_defer() and enable_wgrad_stream(model) on every run, and set_wgrad_stream(True) when its
# environment asks for the stream experiment; the two experiments behind them (weight-gradient GEMMs on a second stream, one deferred
# multi-tensor fold) were measured slower in round 6 and removed: profiles/wgrad_experiments_retired.md.  The names stay so that the
# benchmark runs unchanged.
def set_fold_defer(on):
    pass


def enable_wgrad_stream(module, on=True):
    return False


def set_wgrad_stream(on):
    if on:
        raise lib.FiberHipError("the weight-gradient stream experiment was retired (measured slower in round 6): "
                                "profiles/wgrad_experiments_retired.md has its numbers")


def wgrad(dh, x2, want_bias=False, row_mask=None, scale=1.0, row_map=None):
    """dW[N,K] = dh[M,N]^T . x2[M,K] in fp32 on the hand-written TN kernel (csrc/gemm_tn.hip): both operands are read as
    they lie (row-major, M slow) and transposed on the LDS -> register path; the M reduction is split inside the launch
    (fp32 slabs + one fold).  want_bias: also return the column sums of dh (the bias gradient) from the same pass.
    row_mask / scale: DropPath backward folded in -- samples whose factor in `row_mask` is 0 are skipped, the result is
    multiplied by `scale` (= 1/keep); see droppath_foldable().
    row_map (int32 [N], a permutation): row n of the result (entry n of the bias sums) is written at row_map[n]."""
    M, N = dh.shape
    K = x2.shape[1]
    assert dh.dtype == BF16 and x2.dtype == BF16 and dh.stride(1) == 1 and x2.stride(1) == 1 and x2.shape[0] == M
    dw = torch.empty((N, K), dtype=torch.float32, device=dh.device)
    db = torch.empty(N, dtype=torch.float32, device=dh.device) if want_bias else None
    S = lib.plain("fiber_gemm_tn_splits", M, N, K)
    ws = torch.empty(S * (N * K + N), dtype=torch.float32, device=dh.device) if (S > 1 or row_map is not None) else None   # (the row map is applied by the fold)
    rps = (M // row_mask.numel()) if row_mask is not None else 0
    args = (lib.ptr(dh), lib.ptr(x2), lib.ptr(dw), lib.ptr(db), lib.ptr(ws), M, N, K, dh.stride(0), x2.stride(0), lib.ptr(row_mask), rps,
            float(scale))
    if row_map is not None:
        lib.call("fiber_gemm_tn_rowmap_bf16", *args, lib.ptr(row_map))
    else:
        lib.call("fiber_gemm_tn_bf16", *args)
    return (dw, db) if want_bias else dw


def droppath_foldable(rows, rowscale, rs_value):
    """The DropPath backward factor s_b in {0, 1/keep} can ride in the consumers of the branch gradient instead of a pass of
    its own -- (s dY) W = s (dY W) in the dgrad epilogue, dW = (1/keep) * sum over kept samples in the weight-gradient kernel --
    when the caller knows 1/keep (`rs_value`) and a sample's rows are whole 64-row K tiles (true for Swin stages 0-2 at
    384^2: 9216 / 2304 / 576 tokens per image; stage 3 has 144)."""
    return (rowscale is not None and rs_value and rows % rowscale.numel() == 0
            and (rows // rowscale.numel()) % 64 == 0)


# Column sums that a backward kernel produced together with its output (window attention: the qkv bias gradient).  The
# producer leaves (data_ptr, shape, sums) here; the NEXT linear backward takes the slot -- and uses it only if it is about
# the very tensor it received as dY, unchanged: same address, same shape and the version counter it had at the offer (the
# fan-in add of a second consumer's gradient happens in place, keeps the address and bumps the counter; see the labelled-rows
# slot above).  Every linear backward clears the slot, so it can never be matched against a later tensor that happens to
# reuse the address; a missed hand-over only costs the separate column-sum pass.
_hint_tls = threading.local()          # one hand-over slot per autograd thread (one per device): no cross-thread coupling


def _clear_colsum():
    _hint_tls.slot = None


def _offer_colsum(t2d, sums):
    """Called from inside a backward(): the offer never outlives the autograd pass it was made in."""
    _hint_tls.slot = (t2d.data_ptr(), tuple(t2d.shape), t2d._version, sums)
    torch.autograd.Variable._execution_engine.queue_callback(_clear_colsum)


def _take_colsum(t2d):
    h = getattr(_hint_tls, "slot", None)
    _hint_tls.slot = None
    if h is not None and h[0] == t2d.data_ptr() and h[1] == tuple(t2d.shape) and h[2] == t2d._version:
        return h[3]
    return None


def _dgrad(dh, weight):
    """dX = dY . W on the hand-written NT kernel: the B operand is the transposed bf16 working copy of W ([K, N], one small
    transposing kernel per weight and optimizer step), so the contraction is contiguous on both sides."""
    y, _ = gemm_nt(dh, bf16_weight_t(weight))
    return y


class _Linear(torch.autograd.Function):
    """Returns (y, y32): y32 is the fp32 payload of the output when `res32` (the fp32 payload of the residual) was given."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, act, rowscale, rs_value=None, res32=None):
        shp = x.shape
        x2 = _c(x).view(-1, shp[-1])
        wb = bf16_weight(weight)
        need_pre = bool(act) and any(ctx.needs_input_grad[:3])
        rps = (x2.shape[0] // rowscale.numel()) if rowscale is not None else 0
        oshp = (*shp[:-1], weight.shape[0])
        if res32 is not None:
            assert residual is not None and not act
            y, y32 = gemm_nt(x2, wb, bias, None, 0, False, rowscale, rps, res32=_c(res32).view(-1, weight.shape[0]))
            pre, y32 = None, y32.view(oshp)
            ctx.mark_non_differentiable(y32)
        else:
            r2 = _c(residual).view(-1, weight.shape[0]) if residual is not None else None
            y, pre = gemm_nt(x2, wb, bias, r2, act, need_pre, rowscale, rps)
            y32 = None
        ctx.save_for_backward(x2, weight, pre, rowscale)
        ctx.act, ctx.has_bias, ctx.has_res, ctx.shp, ctx.rs_value = act, bias is not None, residual is not None, shp, rs_value
        return y.view(oshp), y32

    @staticmethod
    def backward(ctx, dy, _dy32=None):
        x2, weight, pre, rowscale = ctx.saved_tensors
        dy2 = _c(dy).view(-1, weight.shape[0])
        dres = dy if ctx.has_res else None
        db = None
        hint = _take_colsum(dy2)
        fold = not ctx.act and dy2.shape[1] % 8 == 0 and droppath_foldable(dy2.shape[0], rowscale, ctx.rs_value)
        if rowscale is not None and not fold:         # branch gradient = per-sample scale * dy, as a pass of its own
            if ctx.has_bias and ctx.needs_input_grad[2] and not ctx.act and dy2.shape[1] % 8 == 0:
                dy2, db = rowscale_colsum(dy2, rowscale)       # ... and the bias gradient from the same pass
            else:
                ds = torch.empty_like(dy2)
                lib.call("fiber_rowscale_add_bf16", None, lib.ptr(dy2), lib.ptr(rowscale), lib.ptr(ds), dy2.numel(),
                         dy2.numel() // rowscale.numel())
                dy2 = ds
        if ctx.act:
            dh, db = gelu_bwd_colsum(dy2, pre)
        else:
            dh = dy2
        need_db = ctx.has_bias and ctx.needs_input_grad[2]
        if fold:                                       # DropPath factor inside the dgrad epilogue and the weight-gradient kernel
            rps = dh.shape[0] // rowscale.numel()
            dx = gemm_nt(dh, bf16_weight_t(weight), None, None, 0, False, rowscale, rps)[0].view(ctx.shp) if ctx.needs_input_grad[0] else None
            dw = db = None
            if ctx.needs_input_grad[1]:
                dw = wgrad(dh, x2, want_bias=need_db, row_mask=rowscale, scale=ctx.rs_value)
                if need_db:
                    dw, db = dw
            elif need_db:
                db = rowscale_colsum(dh, rowscale)[1]
            return dx, dw, db, dres, None, None, None, None
        dx = _dgrad(dh, weight).view(ctx.shp) if ctx.needs_input_grad[0] else None
        if need_db and db is None and hint is not None and dh is dy2:
            db = hint                                  # produced by the kernel that wrote dy (window attention backward)
        want = need_db and db is None                  # otherwise the bias gradient rides in the weight-gradient pass
        dw = None
        if ctx.needs_input_grad[1]:
            dw = wgrad(dh, x2, want_bias=want)
            if want:
                dw, db = dw
        elif want:
            db = colsum(dh)
        if not need_db:
            db = None
        return dx, dw, db, dres, None, None, None, None


def linear(x, weight, bias=None, residual=None, act=None, rowscale=None, rowscale_value=None):
    """nn.Linear with fused bias / exact GELU / residual, forward and both backward GEMMs on the hand-written kernels.
    A library GEMM is used only for shapes the tile kernels do not cover (N % 8 != 0, e.g. the 2-way ITM head, or K % 8 != 0)."""
    N, K = weight.shape
    if (N % 8) or (K % 8):                                 # no backbone linear has such a shape; odd test / head shapes only
        _note_lib_site()
        y = _LibLinear.apply(x, weight.to(BF16), bias.to(BF16) if bias is not None else None)
        if act:
            y = torch.nn.functional.gelu(y)
        assert rowscale is None
        return y + residual if residual is not None else y
    y, y32 = _Linear.apply(x, weight, bias, residual, ACT_GELU if act else 0, rowscale, rowscale_value, f32_of(residual))
    return with_f32(y, y32)


class _MLP(torch.autograd.Function):
    """y = [rowscale *] (fc2(gelu(fc1(x)))) + residual  (timm Mlp inside a Swin block / RoBERTa intermediate+output).

    Forward: two MFMA GEMMs (bias+GELU epilogue saving the pre-activation; bias+DropPath scale+residual epilogue).
    Backward: dH = (dY . W2) * gelu'(H) is ONE hand-written GEMM whose epilogue applies the GELU derivative to the saved
    pre-activation (and the DropPath factor of the branch) -- dG never exists in HBM and the separate gelu_bwd pass over the
    4C-wide tensor disappears.  dX = dH . W1 runs on the same NT kernel family (transposed working copy of W1), dW1 / dW2 and
    both bias gradients on the TN kernel (csrc/gemm_tn.hip); no library GEMM is involved."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, residual, rowscale, rs_value=None, res32=None):
        shp = x.shape
        x2 = _c(x).view(-1, shp[-1])
        need_bwd = any(ctx.needs_input_grad[:5])            # inference (no_grad / frozen): the pre-activation copy is not stored
        g, h = gemm_nt(x2, bf16_weight(w1), b1, None, ACT_GELU, need_bwd)
        rps = (x2.shape[0] // rowscale.numel()) if rowscale is not None else 0
        oshp = (*shp[:-1], w2.shape[0])
        if res32 is not None:                         # fp32 residual stream: (bf16 shadow, fp32 payload)
            y, y32 = gemm_nt(g, bf16_weight(w2), b2, None, 0, False, rowscale, rps, res32=_c(res32).view(-1, w2.shape[0]))
            y32 = y32.view(oshp)
            ctx.mark_non_differentiable(y32)
        else:
            r2 = _c(residual).view(-1, w2.shape[0]) if residual is not None else None
            y, _ = gemm_nt(g, bf16_weight(w2), b2, r2, 0, False, rowscale, rps)
            y32 = None
        if need_bwd:
            ctx.save_for_backward(x2, w1, w2, h, g, rowscale)
        ctx.has_res, ctx.shp, ctx.rs_value = residual is not None, shp, rs_value
        return y.view(oshp), y32

    @staticmethod
    def backward(ctx, dy, _dy32=None):
        dres = dy if ctx.has_res else None
        if not ctx.saved_tensors:                      # frozen block on a trainable stream: only the residual needs a gradient
            return (None,) * 5 + (dres, None, None, None)
        x2, w1, w2, h, g, rowscale = ctx.saved_tensors
        dy2 = _c(dy).view(-1, w2.shape[0])
        db2 = None
        C, C4 = dy2.shape[1], h.shape[1]
        # (dY.W2^T)*gelu'(H) + fc1 bias gradient as ONE hand-written GEMM instead of dgrad + gelu_bwd_colsum, wherever the shape allows.
        # tools/op_bench.py 512 mlpbwd: 3866 vs 4294 us at C=128, 2084 vs 2369 at C=256, 1284 vs 1394 at C=512 (round 2); since round 4
        # (both wave groups of the q8 kernel in the epilogue together, +5-12 %) at C=1024 too: 275.1 / 275.6 -> 274.5 / 274.7 ms per step.
        fused = C % 64 == 0 and C4 % 8 == 0
        fold = fused and dy2.shape[1] % 8 == 0 and droppath_foldable(dy2.shape[0], rowscale, ctx.rs_value)
        rs_arg, rps, mask, scale = None, 0, None, 1.0
        if fold:                                       # DropPath factor rides in the gelu' GEMM epilogue and the wgrad kernel
            rs_arg, rps, mask, scale = rowscale, dy2.shape[0] // rowscale.numel(), rowscale, ctx.rs_value
        elif rowscale is not None:
            if dy2.shape[1] % 8 == 0:
                dy2, db2 = rowscale_colsum(dy2, rowscale)      # DropPath backward + fc2 bias gradient in one pass
            else:
                ds = torch.empty_like(dy2)
                lib.call("fiber_rowscale_add_bf16", None, lib.ptr(dy2), lib.ptr(rowscale), lib.ptr(ds), dy2.numel(),
                         dy2.numel() // rowscale.numel())
                dy2 = ds
        if fused:
            dh, _ = gemm_nt(dy2, bf16_weight_t(w2), None, None, ACT_GELU_BWD, False, rs_arg, rps, aux=h)
            db1 = None
        else:                                         # shapes the DMA kernel does not cover (e.g. Swin-T C=96)
            dh, db1 = gelu_bwd_colsum(_dgrad(dy2, w2), h)
        if db2 is None:
            dw2, db2 = wgrad(dy2, g, want_bias=True, row_mask=mask, scale=scale)
        else:
            dw2 = wgrad(dy2, g)
        dx = _dgrad(dh, w1).view(ctx.shp)
        if db1 is None:
            dw1, db1 = wgrad(dh, x2, want_bias=True)   # fc1 bias gradient = column sums of dH, from the same pass
        else:
            dw1 = wgrad(dh, x2)
        return dx, dw1, db1, dw2, db2, dres, None, None, None


def mlp(x, w1, b1, w2, b2, residual=None, rowscale=None, rowscale_value=None):
    y, y32 = _MLP.apply(x, w1, b1, w2, b2, residual, rowscale, rowscale_value, f32_of(residual))
    return with_f32(y, y32)


# ---- LayerNorm + Mlp + DropPath + residual as one kernel per direction (csrc/mlp_rows.hip; Swin stages with C = 128 / 256) -------------
_fa_perms = {}


def _fa_perm(K, device):
    """Column order of the kernel's weight copies: position p holds logical index p with bits 2 and 3 swapped (mlp_rows.hip)."""
    key = (K, device)
    if key not in _fa_perms:
        i = torch.arange(K, device=device)
        _fa_perms[key] = (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1)
    return _fa_perms[key]


def _fa(m16):
    return m16[:, _fa_perm(m16.shape[1], m16.device)].contiguous()


def _ln_mlp_weights(gamma, beta, w1, b1, w2):
    """(w1p, b1p, w2p, w2tp, w1tp): LayerNorm's affine part folded into fc1 (W1' = W1 diag(gamma), b1' = b1 + W1 beta, formed in
    fp32, ONE bf16 rounding); the copies whose K dimension is the hidden one (w2p, w1tp) in the kernel's K order; rebuilt when any of
    the five parameters changes."""
    key = ("LNMLP", id(w1))
    five = (gamma, beta, w1, b1, w2)
    stamp = tuple(_stamp(t) for t in five)
    hit = _cache_get(key, w1)
    # the entry is keyed by w1 alone, so it remembers (weakly) WHICH five parameters it was built from: a replaced gamma with the
    # same version and generation is not a hit
    if hit is not None and hit[0] == stamp and all(r() is t for r, t in zip(hit[1][5], five)) and hit[1][0].device == w1.device:
        return hit[1][:5]
    with torch.no_grad():
        w1f = w1.detach().float()
        w1p16 = (w1f * gamma.detach().float()[None, :]).to(BF16)
        b1p = torch.addmv(b1.detach().float(), w1f, beta.detach().float()).contiguous()
        w2_16 = w2.detach().to(BF16)
        val = (w1p16.contiguous(), b1p, _fa(w2_16), w2_16.t().contiguous(), _fa(w1p16.t()), tuple(weakref.ref(t) for t in five))
    _cache_put(key, stamp, val, w1)
    return val[:5]


# widths the fused kernels are USED at (they exist for 128 and 256).  Measured at 512 images,
# forward + backward (tools/lnmlp_bench.py, gpurun_out/r06_lnmlp_bench_5.log): C = 128 9.24 ms against 11.11 ms for the separate kernels,
# C = 256 6.68 against 6.12 (one wave per SIMD at that width: nothing runs under its GELU arithmetic) -- so 128 only.
_LN_MLP_WIDTHS = (128,)


def ln_mlp_eligible(x, C):
    return C in _LN_MLP_WIDTHS and C in (128, 256) and x.is_cuda and x.dtype == BF16 and f32_of(x) is None


class _LnMlp(torch.autograd.Function):
    """y = x + rowscale * Mlp(LN(x))  (swin_transformer.py:391) on csrc/mlp_rows.hip: the forward reads x, writes y and (when a
    backward will follow) gelu(H) -- no LayerNorm output, no pre-activation in HBM; the backward recomputes the pre-activation from
    x, returns dx (LayerNorm backward and residual gradient included) and hands dH / xhat to the fc1 weight-gradient GEMM.
    The LayerNorm's gamma / beta ride in the fc1 weight copy, so their gradients come out of dW1' and db1:
    dW1 = dW1' diag(gamma) + db1 (x) beta, dgamma = colsum(dW1' * W1), dbeta = W1^T db1."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, w1, b1, w2, b2, rowscale, rs_value):
        shp = x.shape
        C = shp[-1]
        x2 = _c(x).view(-1, C)
        M = x2.shape[0]
        w1p, b1p, w2p, _, _ = _ln_mlp_weights(gamma, beta, w1, b1, w2)
        y = torch.empty_like(x2)
        need_bwd = any(ctx.needs_input_grad[:8])
        g = torch.empty((M, 4 * C), dtype=BF16, device=x2.device) if need_bwd else None    # gelu(H): the fc2 weight gradient's operand
        rps = M // rowscale.numel() if rowscale is not None else 0
        lib.call("fiber_ln_mlp_fwd_bf16", lib.ptr(x2), lib.ptr(w1p), lib.ptr(b1p), lib.ptr(w2p), lib.ptr(b2.detach()), lib.ptr(rowscale),
                 lib.ptr(y), lib.ptr(g), M, C, rps, float(eps))
        if need_bwd:
            ctx.save_for_backward(x2, gamma, beta, w1, b1, w2, rowscale, g)
        ctx.eps, ctx.shp, ctx.rs_value = float(eps), shp, rs_value
        return y.view(shp)

    @staticmethod
    def backward(ctx, dy):
        x2, gamma, beta, w1, b1, w2, rowscale, g = ctx.saved_tensors
        M, C = x2.shape
        H = 4 * C
        dy2 = _c(dy).view(M, C)
        w1p, b1p, _, w2tp, w1tp = _ln_mlp_weights(gamma, beta, w1, b1, w2)
        dx = torch.empty_like(x2)
        dh = torch.empty((M, H), dtype=BF16, device=x2.device)
        xhat = torch.empty_like(x2)
        rps = M // rowscale.numel() if rowscale is not None else 0
        lib.call("fiber_ln_mlp_bwd_bf16", lib.ptr(x2), lib.ptr(dy2), lib.ptr(w1p), lib.ptr(b1p), lib.ptr(w2tp), lib.ptr(w1tp),
                 lib.ptr(rowscale), lib.ptr(dx), lib.ptr(dh), lib.ptr(xhat), M, C, rps, ctx.eps)
        w1f, gf, bf_ = w1.detach().float(), gamma.detach().float(), beta.detach().float()
        dw1p, db1 = wgrad(dh, xhat, want_bias=True)
        # gradients of LayerNorm's gamma / beta and of W1 out of dW1' (xn = xhat gamma + beta feeds fc1)
        dgamma, dbeta, dw1 = (dw1p * w1f).sum(0), torch.mv(w1f.t(), db1), torch.addcmul(torch.outer(db1, bf_), dw1p, gf[None, :])
        del dh, xhat, dw1p
        if rowscale is None:
            dw2, db2 = wgrad(dy2, g, want_bias=True)
        elif droppath_foldable(M, rowscale, ctx.rs_value):
            dw2, db2 = wgrad(dy2, g, want_bias=True, row_mask=rowscale, scale=ctx.rs_value)
        else:
            dys, db2 = rowscale_colsum(dy2, rowscale)
            dw2 = wgrad(dys, g)
        return dx.view(ctx.shp), dgamma, dbeta, None, dw1, db1, dw2, db2, None, None


def ln_mlp(x, gamma, beta, eps, w1, b1, w2, b2, rowscale=None, rowscale_value=None):
    """x + DropPath(Mlp(LayerNorm(x))) of a Swin block; the fused kernels when ln_mlp_eligible(x, C), else layernorm_res + mlp."""
    if ln_mlp_eligible(x, x.shape[-1]) and w1.shape[0] == 4 * x.shape[-1]:
        return _LnMlp.apply(x, gamma, beta, eps, w1, b1, w2, b2, rowscale, rowscale_value)
    v, r = layernorm_res(x, gamma, beta, eps)
    return mlp(v, w1, b1, w2, b2, residual=r, rowscale=rowscale, rowscale_value=rowscale_value)


def _ln_fwd(x2, x32, gamma, beta, eps, want_f32):
    """LayerNorm rows of x2 (bf16) or of its fp32 payload x32 -> (y bf16, y32 or None, mean, rstd)."""
    rows, C = x2.shape
    y = torch.empty((rows, C), dtype=BF16, device=x2.device)
    y32 = torch.empty((rows, C), dtype=torch.float32, device=x2.device) if want_f32 else None
    mean = torch.empty(rows, dtype=torch.float32, device=x2.device)
    rstd = torch.empty_like(mean)
    if x32 is None and not want_f32:
        lib.call("fiber_layernorm_fwd_bf16", lib.ptr(x2), lib.ptr(gamma), lib.ptr(beta), lib.ptr(y), lib.ptr(mean), lib.ptr(rstd), rows, C, eps)
    else:
        src = x32 if x32 is not None else x2
        lib.call("fiber_layernorm_fwd_stream", lib.ptr(src), lib.ptr(gamma), lib.ptr(beta), lib.ptr(y), lib.ptr(y32), lib.ptr(mean),
                 lib.ptr(rstd), rows, C, eps, 1 if x32 is not None else 0)
    return y, y32, mean, rstd


def _ln_bwd(dy2, xs, is32, gamma, mean, rstd, dr2):
    """LayerNorm backward from the saved input xs (bf16, or fp32 when is32); dr2: residual-path gradient added into dx."""
    rows, C = dy2.shape
    dx = torch.empty((rows, C), dtype=BF16, device=dy2.device)
    dg = torch.empty(C, dtype=torch.float32, device=dy2.device)
    db = torch.empty_like(dg)
    ws = torch.empty(lib.plain("fiber_layernorm_bwd_grid", rows) * 8 * C, dtype=torch.float32, device=dy2.device)
    if is32:
        lib.call("fiber_layernorm_bwd_stream", lib.ptr(dy2), lib.ptr(xs), lib.ptr(gamma), lib.ptr(mean), lib.ptr(rstd), lib.ptr(dr2),
                 lib.ptr(dx), lib.ptr(dg), lib.ptr(db), lib.ptr(ws), rows, C, 1)
    else:
        lib.call("fiber_layernorm_bwd_bf16", lib.ptr(dy2), lib.ptr(xs), lib.ptr(gamma), lib.ptr(mean), lib.ptr(rstd), lib.ptr(dr2),
                 lib.ptr(dx), lib.ptr(dg), lib.ptr(db), lib.ptr(ws), rows, C)
    return dx, dg, db


class _LayerNorm(torch.autograd.Function):
    """(LN(x), fp32 copy of it or None).  x32: fp32 payload of x (the fp32 residual stream); want_f32: also return the output in
    fp32 (post-LN text stack: the LayerNorm output is the next residual)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, x32=None, want_f32=False):
        C = x.shape[-1]
        x2 = _c(x).view(-1, C)
        xs = _c(x32).view(-1, C) if x32 is not None else None
        y, y32, mean, rstd = _ln_fwd(x2, xs, gamma, beta, eps, want_f32)
        ctx.save_for_backward(xs if xs is not None else x2, gamma, mean, rstd)
        ctx.is32 = xs is not None
        if y32 is not None:
            y32 = y32.view(x.shape)
            ctx.mark_non_differentiable(y32)
        return y.view(x.shape), y32

    @staticmethod
    def backward(ctx, dy, _dy32=None):
        xs, gamma, mean, rstd = ctx.saved_tensors
        dx, dg, db = _ln_bwd(_c(dy).view(xs.shape), xs, ctx.is32, gamma, mean, rstd, None)
        return dx.view(dy.shape), dg, db, None, None, None


def layernorm(x, gamma, beta, eps=1e-5, want_f32=False):
    """LayerNorm over the last dim.  Reads the fp32 payload of a stream tensor when it has one.  want_f32 attaches the output's own fp32
    payload: only where the OUTPUT starts or continues a residual stream (patch-embedding norm, the post-LN text stack: those callers ask
    for it).  The pre-LN consumers and the final norms do not -- a payload nothing reads as a residual is an fp32 copy written for nothing,
    and it would make downstream ops treat their input as a stream."""
    x32 = f32_of(x)
    y, y32 = _LayerNorm.apply(x, gamma, beta, eps, x32, bool(want_f32))
    return with_f32(y, y32)


class _LayerNormRes(torch.autograd.Function):
    """(LN(x), x): the second output is x itself, to be used for the residual connection.  Its incoming gradient is
    added inside the LayerNorm backward kernel, so autograd never launches a separate activation-sized add."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, x32=None):
        C = x.shape[-1]
        x2 = _c(x).view(-1, C)
        xs = _c(x32).view(-1, C) if x32 is not None else None
        y, _, mean, rstd = _ln_fwd(x2, xs, gamma, beta, eps, False)
        ctx.save_for_backward(xs if xs is not None else x2, gamma, mean, rstd)
        ctx.is32 = xs is not None
        return y.view(x.shape), x2.view(x.shape)

    @staticmethod
    def backward(ctx, dy, dres):
        xs, gamma, mean, rstd = ctx.saved_tensors
        rows, C = xs.shape
        if dy is None:
            return dres, None, None, None, None
        dr2 = _c(dres).view(rows, C) if dres is not None else None
        dx, dg, db = _ln_bwd(_c(dy).view(rows, C), xs, ctx.is32, gamma, mean, rstd, dr2)
        return dx.view(dy.shape), dg, db, None, None


def layernorm_res(x, gamma, beta, eps=1e-5):
    """Returns (LN(x), x_for_residual); the residual keeps x's fp32 payload."""
    x32 = f32_of(x)
    y, r = _LayerNormRes.apply(x, gamma, beta, eps, x32)
    return y, with_f32(r, x32)


class _PatchMergeLN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, H, W, eps, x32=None):
        B, L, C = x.shape
        xs = _c(x32) if x32 is not None else _c(x)
        rows = B * (H // 2) * (W // 2)
        y = torch.empty((B, rows // B, 4 * C), dtype=BF16, device=x.device)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        if x32 is not None:
            lib.call("fiber_patch_merge_ln_fwd_stream", lib.ptr(xs), lib.ptr(gamma), lib.ptr(beta), lib.ptr(y), lib.ptr(mean), lib.ptr(rstd),
                     B, H, W, C, eps, 1)
        else:
            lib.call("fiber_patch_merge_ln_fwd_bf16", lib.ptr(xs), lib.ptr(gamma), lib.ptr(beta), lib.ptr(y), lib.ptr(mean), lib.ptr(rstd), B, H, W, C, eps)
        ctx.save_for_backward(xs, gamma, mean, rstd)
        ctx.dims, ctx.is32 = (B, H, W, C), x32 is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        xs, gamma, mean, rstd = ctx.saved_tensors
        B, H, W, C = ctx.dims
        rows = B * (H // 2) * (W // 2)
        dy = _c(dy)
        dx = torch.empty(xs.shape, dtype=BF16, device=dy.device)
        dg = torch.empty(4 * C, dtype=torch.float32, device=dy.device)
        db = torch.empty_like(dg)
        ws = torch.empty(lib.plain("fiber_layernorm_bwd_grid", rows) * 8 * 4 * C, dtype=torch.float32, device=dy.device)
        if ctx.is32:
            lib.call("fiber_patch_merge_ln_bwd_stream", lib.ptr(dy), lib.ptr(xs), lib.ptr(gamma), lib.ptr(mean), lib.ptr(rstd), lib.ptr(dx),
                     lib.ptr(dg), lib.ptr(db), lib.ptr(ws), B, H, W, C, 1)
        else:
            lib.call("fiber_patch_merge_ln_bwd_bf16", lib.ptr(dy), lib.ptr(xs), lib.ptr(gamma), lib.ptr(mean), lib.ptr(rstd), lib.ptr(dx),
                     lib.ptr(dg), lib.ptr(db), lib.ptr(ws), B, H, W, C)
        return dx, dg, db, None, None, None, None


def patch_merge_ln(x, gamma, beta, H, W, eps=1e-5):
    return _PatchMergeLN.apply(x, gamma, beta, H, W, eps, f32_of(x))


class _WindowAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, bias_table, B, H, W, heads, ws, shift, head_major):
        C = qkv.shape[-1] // 3
        qkv = _c(qkv)
        rows = B * H * W
        o = torch.empty((rows, C), dtype=BF16, device=qkv.device)
        lse = torch.empty((rows, heads), dtype=torch.float32, device=qkv.device)
        lib.call("fiber_window_attn_fwd_bf16", lib.ptr(qkv), lib.ptr(bias_table), lib.ptr(o), lib.ptr(lse), B, H, W, C, heads, ws, shift, head_major)
        ctx.save_for_backward(qkv, bias_table, o, lse)
        ctx.dims = (B, H, W, C, heads, ws, shift, head_major)
        return o.view(B, H * W, C)

    @staticmethod
    def backward(ctx, do):
        qkv, bias_table, o, lse = ctx.saved_tensors
        B, H, W, C, heads, ws, shift, head_major = ctx.dims
        do = _c(do)
        rows, N = B * H * W, ws * ws
        dqkv = torch.empty_like(qkv)
        dtab = torch.empty_like(bias_table)
        delta = torch.empty((rows, heads), dtype=torch.float32, device=do.device)
        nz = lib.plain("fiber_window_attn_bwd_slices", rows // N, heads)
        part = torch.empty(nz * heads * N * N, dtype=torch.float32, device=do.device)
        # Column sums of dqkv (= bias gradient of the qkv linear) CAN come out of the same passes (round 2: -5 ms per step against a pass of
        # their own over dqkv).  Round 4: they cost the window backward 6-12 % (tools/win_colsum_probe.py: stage 2 780 -> 730 us, stage 0
        # 2950 -> 2610), while the weight-gradient kernel of the qkv linear now takes its bias sums for ~1 % -- so by default the qkv linear's
        # backward asks that kernel (no offer is made); FIBER_WIN_COLSUM=1 restores the in-kernel sums.
        cs_rows = lib.plain("fiber_window_attn_colsum_rows", rows // N, heads, ws) if _WIN_COLSUM else 0
        csum = torch.empty(3 * C, dtype=torch.float32, device=do.device) if cs_rows else None
        cs_ws = torch.empty(cs_rows * 3 * C, dtype=torch.float32, device=do.device) if cs_rows else None
        lib.call("fiber_window_attn_bwd_bf16", lib.ptr(qkv), lib.ptr(bias_table), lib.ptr(o), lib.ptr(do), lib.ptr(lse), lib.ptr(dqkv),
                 lib.ptr(dtab), lib.ptr(delta), lib.ptr(part), lib.ptr(csum), lib.ptr(cs_ws), B, H, W, C, heads, ws, shift, head_major)
        if csum is not None:
            _offer_colsum(dqkv.view(-1, 3 * C), csum)
        return dqkv, dtab, None, None, None, None, None, None, None


def window_attention(qkv, bias_table, B, H, W, heads, ws, shift, head_major=False):
    """qkv [B, H*W, 3C] in image-token order -> attention output [B, H*W, C] (shift/partition/reverse folded in).
    head_major: qkv channels are [heads][3][32] (see linear_qkv_head_major) instead of the reference [3][heads][32]."""
    return _WindowAttn.apply(qkv, bias_table, B, H, W, heads, ws, shift, int(head_major))


def head_major_supported(ws):
    """The one-chunk window kernels (N = ws*ws <= 160, WIN_SMALL_N of csrc/win_attn.hip's win_plan()) are the sizes the model runs head-major."""
    return ws * ws <= 160


_perm_cache = {}


def _qkv_perm(C, heads, device):
    """perm[r'] = r: row r' = h*96 + which*32 + d of the head-major projection is row r = which*C + h*32 + d of qkv.weight."""
    key = (C, heads, str(device))
    if key not in _perm_cache:
        h, which, d = torch.meshgrid(torch.arange(heads), torch.arange(3), torch.arange(32), indexing="ij")
        perm = (which * C + h * 32 + d).reshape(-1).to(device)
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(3 * C, device=device)
        _perm_cache[key] = (perm, inv)
    return _perm_cache[key]


def _qkv_perm32(C, heads, device):
    key = ("i32", C, heads, str(device))
    if key not in _perm_cache:
        _perm_cache[key] = _qkv_perm(C, heads, device)[0].to(torch.int32).contiguous()
    return _perm_cache[key]


def _head_major_weights(weight, bias, heads):
    """(wp, bp, wpt): the bf16 weight of a qkv projection with its rows in [heads][3][32] order, the fp32 bias in that order, the transpose
    of the first.  The entry remembers (weakly) WHICH bias it was built from: a replaced one is a miss, like a changed one."""
    key = ("HM", id(weight))
    hit = _cache_get(key, weight)
    if hit is None or hit[0] != (_stamp(weight), _stamp(bias)) or hit[1][3]() is not bias or hit[1][0].device != weight.device:
        perm = _qkv_perm(weight.shape[1], heads, weight.device)[0]
        wp = weight.detach()[perm].to(BF16).contiguous()
        _cache_put(key, (_stamp(weight), _stamp(bias)), (wp, bias.detach()[perm].contiguous(), wp.t().contiguous(), weakref.ref(bias), heads), weight)
    return _wcache[key][1][:3]


class _LinearQKVHeadMajor(torch.autograd.Function):
    """qkv = x . W^T + b with the OUTPUT channels reordered to [heads][3][32]: q|k|v of one head become one contiguous
    192-byte run per token, so the per-head gathers of the window-attention kernels use 3/4 of every cache line they touch
    instead of 1/2.  Only the bf16 working copy of the weight is permuted; parameters / gradients keep the reference layout."""

    @staticmethod
    def forward(ctx, x, weight, bias, heads):
        shp = x.shape
        x2 = _c(x).view(-1, shp[-1])
        wp, bp, _ = _head_major_weights(weight, bias, heads)
        y, _ = gemm_nt(x2, wp, bp)
        ctx.save_for_backward(x2, weight)
        ctx.shp, ctx.heads = shp, heads
        return y.view(*shp[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, weight = ctx.saved_tensors
        dy2 = _c(dy).view(-1, weight.shape[0])
        hint = _take_colsum(dy2)
        perm, inv = _qkv_perm(weight.shape[1], ctx.heads, dy.device)
        wp, _, wpt = _wcache[("HM", id(weight))][1][:3]
        dx = gemm_nt(dy2, wpt)[0].view(ctx.shp)
        pmap = _qkv_perm32(weight.shape[1], ctx.heads, dy.device)     # row r' of the head-major gradient is written at row perm[r'] by the kernel
        if hint is not None:
            dw, db = wgrad(dy2, x2, row_map=pmap), hint[inv]
        else:
            dw, db = wgrad(dy2, x2, want_bias=True, row_map=pmap)
        return dx, dw, db, None


def linear_qkv_head_major(x, weight, bias, heads):
    return _LinearQKVHeadMajor.apply(x, weight, bias, heads)


# ---- packed projections ---------------------------------------------------------------------------------------------------------
# q / k / v of RobertaSelfAttention (roberta.py:256-290) and key / value of the t2i cross-attention are separate nn.Linear modules
# (separate state-dict keys) applied to the SAME input.  Here they run as ONE GEMM: the bf16 working copies of the member weights
# are row slices of one [sum N, K] buffer (registered in the weight cache as the members' own working copies, so the fused
# optimizer kernel rewrites the packed buffer in place), its transposed copy is one entry of the multi-tensor transpose, and the
# member BIASES (fp32 parameters) are re-pointed at slices of one fp32 buffer (same values, same Parameter objects, shared
# storage) -- no per-step gather of either.  One forward GEMM, one dgrad, one wgrad (+ fold) instead of three each, and no
# autograd fan-in adds of the three input gradients.
_packs = {}


def _pack_views_ok(pk, ws):
    off = 0
    for w, n in zip(ws, pk["Ns"]):
        hit = _cache_get(id(w), w)
        if hit is None or hit[1].data_ptr() != pk["plain"].data_ptr() + off * pk["K"] * 2:
            return False
        off += n
    return True


def _pack_get(weights, biases):
    key = tuple(id(w) for w in weights)
    pk = _packs.get(key)
    dev = weights[0].device
    if pk is None or pk["plain"].device != dev or any(r() is not w for r, w in zip(pk["refs"], weights)):
        Ns, K = [w.shape[0] for w in weights], weights[0].shape[1]
        pk = {"plain": torch.empty((sum(Ns), K), dtype=BF16, device=dev), "t": torch.empty((K, sum(Ns)), dtype=BF16, device=dev),
              "refs": [weakref.ref(w, lambda _r, k=key: _packs.pop(k, None)) for w in weights], "Ns": Ns, "K": K, "t_stamp": None,
              "bias": None}
        _packs[key] = pk
    if not _pack_views_ok(pk, weights):                     # (re-)register the members' working copies as views of the pack
        off = 0
        for w, n in zip(weights, pk["Ns"]):
            view = pk["plain"][off:off + n]
            view.copy_(w.detach())
            _cache_put(id(w), _stamp(w), view, w)
            off += n
        pk["t_stamp"] = None
    else:
        for w in weights:                                   # stale member (parameter changed outside the fused optimizer)
            if _cache_get(id(w), w)[0] != _stamp(w):
                bf16_weight(w)                              # in-place refresh of the view
                pk["t_stamp"] = None
    stamps = tuple(_stamp(w) for w in weights)
    if pk["t_stamp"] != stamps:
        pk["t"].copy_(pk["plain"].t())
        pk["t_stamp"] = stamps
    if biases[0] is not None:
        bp, off, ok = pk["bias"], 0, pk["bias"] is not None
        for b, n in zip(biases, pk["Ns"]):
            ok = ok and b.data_ptr() == bp.data_ptr() + off * 4
            off += n
        if not ok:                                          # first use / the parameters moved (model.to, load with assign)
            if any(b.dtype != torch.float32 for b in biases):   # the members' .data is re-pointed at the pack: it must keep their dtype
                raise TypeError("linear_packed: biases must be fp32 masters (got " + ", ".join(str(b.dtype) for b in biases) + ")")
            with torch.no_grad():
                bp = torch.cat([b.detach().reshape(-1) for b in biases])
                off = 0
                for b, n in zip(biases, pk["Ns"]):
                    if b.is_cuda:
                        # the cat above may still be QUEUED on this (second) stream when the old storage -- allocated on the default
                        # stream -- is dropped here: without this the other stream's next allocation reuses and overwrites it first
                        b.data.record_stream(torch.cuda.current_stream(b.device))
                    b.data = bp[off:off + n]                # same values, shared storage: optimizer updates land in the pack
                    off += n
            pk["bias"] = bp
    return pk


class _LinearPacked(torch.autograd.Function):
    """fork: the node also returns an ALIAS of its input for the input's other consumer (the image block that follows the text layer whose t2i
    keys / values this projection forms).  The other consumer's gradient then arrives HERE instead of at autograd's fan-in, and the dX GEMM adds it
    in its residual epilogue: one read of that gradient instead of a three-tensor `add` pass over [B*L, C] (8 of them per step, 0.9 GB each at stage 2)."""

    @staticmethod
    def forward(ctx, x, n, fork, *wb):
        weights, biases = wb[0::2], wb[1::2]
        pk = _pack_get(weights, biases)
        shp = x.shape
        x2 = _c(x).view(-1, shp[-1])
        y, _ = gemm_nt(x2, pk["plain"], pk["bias"])
        ctx.save_for_backward(x2)
        ctx.pk, ctx.shp, ctx.has_bias = pk, shp, biases[0] is not None
        y = y.view(*shp[:-1], pk["plain"].shape[0])
        return (y, x.view_as(x)) if fork else y

    @staticmethod
    def backward(ctx, dy, dalias=None):
        (x2,) = ctx.saved_tensors
        pk = ctx.pk
        dy2 = _c(dy).view(-1, pk["plain"].shape[0])
        _take_colsum(dy2)
        dx = None
        if ctx.needs_input_grad[0]:
            if dalias is not None:
                da2 = _c(dalias).view(-1, ctx.shp[-1])
                ones = _ones_rows(dy2.device)
                dx = gemm_nt(dy2, pk["t"], None, da2, rowscale=ones, rows_per_sample=dy2.shape[0])[0].view(ctx.shp)   # dY W + the alias' gradient
            else:
                dx = gemm_nt(dy2, pk["t"])[0].view(ctx.shp)
        out = wgrad(dy2, x2, want_bias=ctx.has_bias)
        dw, db = out if ctx.has_bias else (out, None)
        grads, off = [], 0
        for n in pk["Ns"]:
            grads += [dw[off:off + n], db[off:off + n] if db is not None else None]
            off += n
        return (dx, None, None, *grads)


_ones_cache = {}


def _ones_rows(device):
    t = _ones_cache.get(device)
    if t is None:
        t = _ones_cache[device] = torch.ones(1, dtype=torch.float32, device=device)
    return t


def linear_packed(x, linears, fork_sink=None):
    """[x W0^T + b0 | x W1^T + b1 | ...] for nn.Linear-like (weight, bias) pairs that share the input: one GEMM (see above).
    Falls back to separate GEMMs + cat for shapes the tile kernels do not cover."""
    weights = [w for w, _ in linears]
    biases = [b for _, b in linears]
    K = weights[0].shape[1]
    if (any(w.shape[1] != K or w.shape[0] % 8 for w in weights) or K % 8
            or any((b is None) != (biases[0] is None) for b in biases)):
        return torch.cat([linear(x, w, b) for w, b in linears], dim=-1)
    flat = [t for pair in zip(weights, biases) for t in pair]
    if fork_sink is not None and torch.is_grad_enabled() and x.requires_grad and f32_of(x) is None and x.dtype == BF16:
        y, alias = _LinearPacked.apply(x, len(weights), True, *flat)
        fork_sink.append(alias)
        return y
    return _LinearPacked.apply(x, len(weights), False, *flat)


def _ld(t):
    assert t.dim() == 2 and t.stride(1) == 1
    return t.stride(0)


def _mha_fwd(q, k, v, kmask, B, heads, scale, p_drop, seed, base, causal=False):
    """fiber_mha_fwd_bf16 (causal: fiber_mha_causal_fwd_bf16) on q [B*Lq, heads*D], k / v [B*Lk, heads*D], possibly column views of a
    packed projection -> (o, lse)"""
    o = torch.empty(q.shape, dtype=BF16, device=q.device)
    lse = torch.empty((q.shape[0], heads), dtype=torch.float32, device=q.device)
    lib.call("fiber_mha_causal_fwd_bf16" if causal else "fiber_mha_fwd_bf16", lib.ptr(q), lib.ptr(k), lib.ptr(v), lib.ptr(kmask), lib.ptr(o),
             lib.ptr(lse), B, heads, q.shape[0] // B, k.shape[0] // B, q.shape[1] // heads, _ld(q), _ld(k), _ld(v), _ld(o), scale, p_drop,
             seed, base)
    return o, lse


def _mha_bwd(q, k, v, kmask, o, lse, do, dq, dk, dv, B, heads, scale, p_drop, seed, base, causal=False):
    """the backward of _mha_fwd into dq / dk / dv (possibly column views of a packed gradient)"""
    do = _c(do)
    delta = torch.empty((q.shape[0], heads), dtype=torch.float32, device=q.device)
    lib.call("fiber_mha_causal_bwd_bf16" if causal else "fiber_mha_bwd_bf16", lib.ptr(q), lib.ptr(k), lib.ptr(v), lib.ptr(kmask), lib.ptr(o),
             lib.ptr(do), lib.ptr(lse), lib.ptr(dq), lib.ptr(dk), lib.ptr(dv), lib.ptr(delta), B, heads, q.shape[0] // B, k.shape[0] // B,
             q.shape[1] // heads, _ld(q), _ld(k), _ld(v), _ld(o), _ld(do), _ld(dq), _ld(dk), _ld(dv), scale, p_drop, seed, base)


class _MHA(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, kmask, B, heads, scale, p_drop, seed):
        ctx.cfg = (B, heads, scale, p_drop, seed, seed_base_ptr())
        o, lse = _mha_fwd(q, k, v, kmask, *ctx.cfg)
        ctx.save_for_backward(q, k, v, kmask, o, lse)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, kmask, o, lse = ctx.saved_tensors
        dq = torch.empty_like(o)
        dk = torch.empty((k.shape[0], o.shape[1]), dtype=BF16, device=q.device)
        dv = torch.empty_like(dk)
        _mha_bwd(q, k, v, kmask, o, lse, do, dq, dk, dv, *ctx.cfg)
        return dq, dk, dv, None, None, None, None, None, None


def mha(q, k, v, kmask, B, heads, scale, p_drop=0.0, seed=0):
    """softmax(q.k^T*scale + kmask).v per (sample, head); q/k/v are 2-D [B*L, heads*D] bf16, kmask fp32 [B, Lk] or None."""
    if kmask is not None:
        kmask = _c(kmask.view(B, -1).float())
    return _MHA.apply(q, k, v, kmask, B, heads, float(scale), float(p_drop), int(seed))


class _MHAPacked(torch.autograd.Function):
    """mha() on packed projections: mode 0: `a` = [q | k | v] ([B*L, 3*heads*D], self-attention), mode 1: `a` = q, `b` = [k | v].
    The backward kernel writes dq / dk / dv straight into the column blocks of ONE packed gradient per input, so the projection's
    backward is one dgrad + one wgrad and autograd never assembles slices."""

    @staticmethod
    def _views(a, b, mode):
        """the q, k, v column blocks of a packed input (or of its gradient)"""
        C = a.shape[1] // 3
        return (a[:, :C], a[:, C:2 * C], a[:, 2 * C:]) if mode == 0 else (a, b[:, :a.shape[1]], b[:, a.shape[1]:])

    @staticmethod
    def forward(ctx, a, b, kmask, mode, B, heads, scale, p_drop, seed, causal=False):
        a = _c(a)
        b = _c(b) if b is not None else None
        ctx.mode, ctx.cfg = mode, (B, heads, scale, p_drop, seed, seed_base_ptr(), causal)
        o, lse = _mha_fwd(*_MHAPacked._views(a, b, mode), kmask, *ctx.cfg)
        ctx.save_for_backward(a, b, kmask, o, lse)
        return o

    @staticmethod
    def backward(ctx, do):
        a, b, kmask, o, lse = ctx.saved_tensors
        da = torch.empty_like(a)
        db = torch.empty_like(b) if b is not None else None
        _mha_bwd(*_MHAPacked._views(a, b, ctx.mode), kmask, o, lse, do, *_MHAPacked._views(da, db, ctx.mode), *ctx.cfg)
        return da, db, None, None, None, None, None, None, None, None


def mha_qkv_packed(qkv, kmask, B, heads, scale, p_drop=0.0, seed=0, causal=False):
    """Self-attention on a packed projection qkv [B*L, 3*heads*D] = [q | k | v] (linear_packed).  causal=True: key j > query i is
    masked as well (text decoder; L <= 64, kmask [B, L] additive or None)."""
    if kmask is not None and kmask.numel() != qkv.shape[0]:     # e.g. a dense [B, 1, L, L] mask, which view(B, -1) would misread
        raise ValueError(f"mha_qkv_packed: kmask must be an additive [B, L] key mask, got shape {tuple(kmask.shape)}")
    if kmask is not None:
        kmask = _c(kmask.view(B, -1).float())
    return _MHAPacked.apply(qkv, None, kmask, 0, B, heads, float(scale), float(p_drop), int(seed), bool(causal))


def mha_kv_packed(q, kv, kmask, B, heads, scale, p_drop=0.0, seed=0):
    """Cross-attention with the key / value projections packed: q [B*Lq, heads*D], kv [B*Lk, 2*heads*D] = [k | v]."""
    if kmask is not None:
        kmask = _c(kmask.view(B, -1).float())
    return _MHAPacked.apply(q, kv, kmask, 1, B, heads, float(scale), float(p_drop), int(seed))


# ---- single-token attention of the KV-cached caption decoder (csrc/attn_decode.hip): forward only -------------------------------------
DECODE_MAX_LEN = 64          # the causal kernels' own limit
DECODE_MAX_ROWS = 16         # rows (beams) per image the cross kernel serves from one K/V fetch


def _decode_check(name, x, heads, what):
    if x.dim() != 2 or x.stride(1) != 1 or heads < 1 or x.shape[1] % heads or x.shape[1] // heads not in (32, 64):
        raise ValueError(f"{name}: {what} {tuple(x.shape)} strides {x.stride()} for {heads} heads: 2-D rows of heads * (32 | 64) channels")


def _softmax_v(q, K, V, heads, scale, out_dtype, live=None):
    """softmax(scale q.K^T) V per head for one query per row: q [N, C], K / V [N, L, C] -> [N, C]; live bool [N, L]: the keys that count (a
    row without one gives 0) (host restatements)"""
    N, L, C = K.shape
    ct = torch.promote_types(q.dtype, torch.float32)
    q, K, V = (x.to(ct).reshape(*x.shape[:-1], heads, C // heads) for x in (q, K, V))
    s = torch.einsum("nhd,nlhd->nhl", q, K) * scale
    if live is not None:
        s = s.masked_fill(~live[:, None, :], float("-inf"))
        V = torch.where(live[:, :, None, None], V, torch.zeros_like(V))
    p = torch.softmax(s, -1)
    if live is not None:
        p = torch.where(live.any(1)[:, None, None], p, torch.zeros_like(p))
    return torch.einsum("nhl,nlhd->nhd", p, V).reshape(N, C).to(out_dtype)


def _mha_decode_self_host(qkv, cache, anc, t, heads, scale):
    """fiber_mha_decode_self_bf16 on CPU tensors, in torch, the in-place cache append included"""
    N, C = qkv.shape[0], cache.shape[2] // 2
    slots = anc[:, :t].long() if anc is not None else torch.arange(N)[:, None].expand(N, t)
    live = None
    if anc is not None:                                                          # an entry outside [0, N): no key, never dereferenced
        live = (anc[:, :t + 1] >= 0) & (anc[:, :t + 1] < N)
        slots = torch.where(live[:, :t], slots, torch.arange(N)[:, None].expand(N, t))
    past = cache[slots, torch.arange(t)[None, :]]                                # [N, t, 2C]: position j from slot anc[n, j]
    new = qkv[:, C:3 * C]
    kv = torch.cat([past, new[:, None].to(cache.dtype)], 1)                      # position t: the row's own k | v
    o = _softmax_v(qkv[:, :C], kv[..., :C], kv[..., C:], heads, scale, qkv.dtype, live)
    cache[:, t] = new.to(cache.dtype)
    return o


def mha_decode_self(qkv, cache, anc, t, heads, scale):
    """Causal self-attention of ONE new token per row against that row's cache.  qkv [N, 3C] = [q | k | v] of the token at position t
    (linear_packed; any row stride that is a multiple of 8), cache [N slots, Lmax, 2C] = [k | v] per position (one per layer, contiguous),
    anc int32 [N, Lmax] or None.  Stores row n's k | v to cache[n, t] IN PLACE and returns softmax(scale q.K[0..t]).V [N, C], the key and
    value of position j < t read from slot anc[n, j] (slot n without anc), position t taken from qkv: a beam reorder gathers the small anc
    table, never a cache.  A position j <= t whose anc[n, j] is outside [0, N) (-1) is no key, as a padded key under infer_caption's text_masks:
    it is skipped, position t itself included (its k | v are appended all the same); a live position t has anc[n, t] = n; a row without any
    key gives 0.  Nothing beyond position t is read.  Lmax <= 64, head width 32 or 64; no gradient.  On CPU tensors the same in torch."""
    t = int(t)
    if cache.dim() != 3 or cache.shape[2] % 2:
        raise ValueError(f"mha_decode_self: cache {tuple(cache.shape)}: [N, Lmax, 2C]")
    N, Lmax, C = cache.shape[0], cache.shape[1], cache.shape[2] // 2
    if qkv.dim() != 2 or qkv.shape != (N, 3 * C) or qkv.dtype != cache.dtype or qkv.device != cache.device:
        raise ValueError(f"mha_decode_self: qkv {tuple(qkv.shape)} {qkv.dtype} for cache {tuple(cache.shape)} {cache.dtype}: [N, 3C], same type and device")
    _decode_check("mha_decode_self", qkv[:, :C], heads, "q")
    if not 0 <= t < Lmax or Lmax > DECODE_MAX_LEN:
        raise ValueError(f"mha_decode_self: position {t} of {Lmax} (the kernel serves 0 <= t < Lmax <= {DECODE_MAX_LEN})")
    if anc is not None and (anc.shape != (N, Lmax) or anc.dtype != torch.int32 or anc.device != cache.device):
        raise ValueError(f"mha_decode_self: anc {tuple(anc.shape)} {anc.dtype}: int32 [N, Lmax] beside the cache")
    if not cache.is_contiguous():
        raise ValueError("mha_decode_self: the cache is appended in place and must be contiguous")
    if not cache.is_cuda:
        return _mha_decode_self_host(qkv, cache, anc, t, heads, scale)
    if qkv.dtype != BF16:
        raise ValueError(f"mha_decode_self: {qkv.dtype} on the device (bf16)")
    if qkv.stride(0) % 8 or qkv.data_ptr() % 16:
        qkv = _c(qkv)
    if cache.data_ptr() % 16:
        raise ValueError("mha_decode_self: the cache must start on a 16-byte boundary")
    o = torch.empty((N, C), dtype=BF16, device=qkv.device)
    lib.call("fiber_mha_decode_self_bf16", lib.ptr(qkv), lib.ptr(cache), lib.ptr(_c(anc) if anc is not None else None), lib.ptr(o), N, heads,
             C // heads, t, Lmax, qkv.stride(0) if N > 1 else 3 * C, C, float(scale))
    return o


def _mha_decode_cross_host(q, kv, R, heads, scale):
    """fiber_mha_decode_cross_bf16 on CPU tensors, in torch: row n against the K / V of image n // R"""
    C = q.shape[1]
    rep = kv.repeat_interleave(R, 0)
    return _softmax_v(q, rep[..., :C], rep[..., C:], heads, scale, q.dtype)


def mha_decode_cross(q, kv, rows_per_image, heads, scale):
    """Text->image cross-attention of one new token per row: q [N = G * R, C] (any row stride that is a multiple of 8), kv [G, Lk, 2C] =
    [k | v] of each image's tokens as linear_packed(image_tokens, [key, value]) lays it out, image-major and NOT repeated per beam; row n
    belongs to image n // R, R = rows_per_image <= 16.  No mask (the reference passes none at this site), no gradient.  An image's K / V is
    read once for its R rows; a row's output depends neither on R nor on the other rows.  On CPU tensors the same in torch."""
    R = int(rows_per_image)
    _decode_check("mha_decode_cross", q, heads, "q")
    N, C = q.shape
    if kv.dim() != 3 or kv.shape[2] != 2 * C or kv.shape[1] < 1 or kv.dtype != q.dtype or kv.device != q.device:
        raise ValueError(f"mha_decode_cross: kv {tuple(kv.shape)} {kv.dtype} for q {tuple(q.shape)} {q.dtype}: [G, Lk >= 1, 2C], same type and device")
    if not 1 <= R <= DECODE_MAX_ROWS or N != kv.shape[0] * R:
        raise ValueError(f"mha_decode_cross: {N} rows, {kv.shape[0]} images, {R} rows per image (1 <= R <= {DECODE_MAX_ROWS}, N = G * R)")
    if not q.is_cuda:
        return _mha_decode_cross_host(q, kv, R, heads, scale)
    if q.dtype != BF16:
        raise ValueError(f"mha_decode_cross: {q.dtype} on the device (bf16)")
    if q.stride(0) % 8 or q.data_ptr() % 16:
        q = _c(q)
    kv = _c(kv)
    o = torch.empty((N, C), dtype=BF16, device=q.device)
    lib.call("fiber_mha_decode_cross_bf16", lib.ptr(q), lib.ptr(kv), lib.ptr(o), N, R, heads, kv.shape[1], C // heads,
             q.stride(0) if N > 1 else C, C, float(scale))
    return o


_DOT_PARTS = lib.DEFINES["FIBER_DOT_PARTS"]      # workspace floats of fiber_dot_bf16 / the d alpha of fiber_stream_add_bwd


class _ScaleAdd(torch.autograd.Function):
    """out = a + alpha * b with a learnable scalar alpha (alpha_i2t / alpha_t2i)."""

    @staticmethod
    def forward(ctx, a, b, alpha):
        a, b = _c(a), _c(b)
        out = torch.empty_like(a)
        lib.call("fiber_scale_add_bf16", lib.ptr(a), lib.ptr(b), lib.ptr(alpha), 1.0, lib.ptr(out), a.numel())
        ctx.save_for_backward(b, alpha)
        return out

    @staticmethod
    def backward(ctx, dout):
        b, alpha = ctx.saved_tensors
        dout = _c(dout)
        db = torch.empty_like(b)
        lib.call("fiber_scale_add_bf16", None, lib.ptr(dout), lib.ptr(alpha), 1.0, lib.ptr(db), dout.numel())
        dalpha = torch.empty(1, dtype=torch.float32, device=dout.device)
        ws = torch.empty(_DOT_PARTS, dtype=torch.float32, device=dout.device)
        lib.call("fiber_dot_bf16", lib.ptr(dout), lib.ptr(b), lib.ptr(dalpha), lib.ptr(ws), dout.numel())
        return dout, db, dalpha


def scale_add(a, b, alpha):
    return _ScaleAdd.apply(a, b, alpha)


class _Add(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = _c(a), _c(b)
        out = torch.empty_like(a)
        lib.call("fiber_scale_add_bf16", lib.ptr(a), lib.ptr(b), None, 1.0, lib.ptr(out), a.numel())
        return out

    @staticmethod
    def backward(ctx, dout):
        return dout, dout


def add(a, b):
    """Residual add of two same-shape bf16 tensors."""
    return _Add.apply(a, b)


class _StreamAdd(torch.autograd.Function):
    """(out16, out32) = res + rowscale[sample] * (drop_a(a) + alpha * drop_b(b))  -- csrc/elementwise.hip stream_add_kernel."""

    @staticmethod
    def forward(ctx, res, a, b, alpha, rowscale, p_a, seed_a, p_b, seed_b, res32, want32):
        a = _c(a)
        b = _c(b) if b is not None else None
        kind, rsrc = 0, None
        if res32 is not None:
            kind, rsrc = 2, _c(res32)
        elif res is not None:
            kind, rsrc = 1, _c(res)
        out16 = torch.empty_like(a)
        out32 = torch.empty(a.shape, dtype=torch.float32, device=a.device) if want32 else None
        per = (a.numel() // rowscale.numel()) if rowscale is not None else 0
        base = seed_base_ptr()
        lib.call("fiber_stream_add", lib.ptr(rsrc), kind, lib.ptr(a), lib.ptr(b), lib.ptr(alpha), lib.ptr(rowscale), per, float(p_a), int(seed_a),
                 float(p_b), int(seed_b), base, lib.ptr(out32), lib.ptr(out16), a.numel())
        ctx.save_for_backward(b if (alpha is not None and b is not None) else None, alpha, rowscale)
        ctx.cfg = (per, float(p_a), int(seed_a), float(p_b), int(seed_b), base, res is not None, b is not None)
        if out32 is not None:
            ctx.mark_non_differentiable(out32)
        return out16, out32

    @staticmethod
    def backward(ctx, dy, _d32=None):
        b, alpha, rowscale = ctx.saved_tensors
        per, p_a, seed_a, p_b, seed_b, base, has_res, has_b = ctx.cfg
        dy = _c(dy)
        plain_a = rowscale is None and p_a == 0.0                       # d a = dy itself
        da = dy if plain_a else torch.empty_like(dy)
        db = torch.empty_like(dy) if has_b else None
        dalpha = torch.empty(1, dtype=torch.float32, device=dy.device) if (alpha is not None and has_b and ctx.needs_input_grad[3]) else None
        ws = torch.empty(_DOT_PARTS, dtype=torch.float32, device=dy.device) if dalpha is not None else None
        if not plain_a or has_b:
            lib.call("fiber_stream_add_bwd", lib.ptr(dy), lib.ptr(b), lib.ptr(alpha), lib.ptr(rowscale), per, p_a, seed_a, p_b, seed_b, base,
                     None if plain_a else lib.ptr(da), lib.ptr(db), lib.ptr(dalpha), lib.ptr(ws), dy.numel())
        return (dy if has_res else None), da, db, dalpha, None, None, None, None, None, None, None


def stream_add(res, a, b=None, alpha=None, rowscale=None, p_a=0.0, p_b=0.0, training=True):
    """res + rowscale * (dropout_pa(a) + alpha * dropout_pb(b)) in one pass.  `res` may be a stream pair (its fp32 payload is read
    and the result is a pair again), a plain bf16 tensor, or None (with residual_fp32() a NEW stream starts when res is None
    only if the caller attaches it).  Dropout keys are drawn here (one per active dropout, a before b)."""
    p_a = float(p_a) if training else 0.0
    p_b = float(p_b) if (training and b is not None) else 0.0
    seed_a = next_seed() if p_a > 0 else 0
    seed_b = next_seed() if p_b > 0 else 0
    r32 = f32_of(res)
    want32 = r32 is not None or (_RESIDUAL_FP32[0] and res is not None)
    y, y32 = _StreamAdd.apply(res, a, b, alpha, rowscale, p_a, seed_a, p_b, seed_b, r32, want32)
    return with_f32(y, y32)


def stream_bf16(x):
    """The bf16 tensor a GEMM may read for a stream tensor: the shadow itself (every producer on the stream writes one)."""
    return x


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed):
        x = _c(x)
        y = torch.empty_like(x)
        base = seed_base_ptr()
        lib.call("fiber_dropout_bf16", lib.ptr(x), lib.ptr(y), x.numel(), p, seed, base)
        ctx.cfg = (p, seed, base)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _c(dy)
        dx = torch.empty_like(dy)
        lib.call("fiber_dropout_bf16", lib.ptr(dy), lib.ptr(dx), dy.numel(), *ctx.cfg)
        return dx, None, None


# Dropout / DropPath keys.  key = BASE(seed, step) + call-site counter, where the counter restarts at every training step:
#   eager:  the whole key is passed to the kernels by value;
#   graph:  (enable_graph_rng) BASE lives in a device int64 scalar that set_rng_step() rewrites before every replay, the
#           kernels receive only the counter by value + the pointer -- a captured step draws new masks on every replay and
#           the SAME masks an eager run of that step would draw.
_seed_state = {"seed": 0x5EED, "ctr": 0, "step": None, "base_dev": None}
_M64 = (1 << 64) - 1


def _base_value():
    hi, step = _seed_state["seed"], _seed_state["step"]
    if step is None:
        return (hi << 32) & _M64
    hi = (hi ^ ((int(step) >> 12) * 0x9E3779B1)) & 0xFFFFFFFF
    return ((hi << 32) | ((int(step) & 0xFFF) << 20)) & _M64


def _write_base_dev():
    t = _seed_state["base_dev"]
    if t is not None:
        v = _base_value()
        t.fill_(v - (1 << 64) if v >= (1 << 63) else v)    # the bit pattern, through torch's signed int64


def manual_seed(seed):
    """Seed of the dropout / DropPath streams (lightning.seed_everything and the Trainer call this with config["seed"] + rank)."""
    _seed_state["seed"], _seed_state["ctr"], _seed_state["step"] = int(seed) & 0xFFFFFFFF, 0, None
    _seed_state["collate_ctr"] = 0
    _write_base_dev()


def set_rng_step(step):
    """Called once per training step with the optimizer-step index: the per-call-site counter restarts inside a window of
    2^20 keys owned by that step, so a run resumed at step s draws the masks of step s, not those of step 0."""
    if _seed_state["step"] != step:
        _seed_state["step"] = step
        _seed_state["ctr"] = 0
        if _seed_state["base_dev"] is not None and not torch.cuda.is_current_stream_capturing():
            _write_base_dev()


def enable_graph_rng(device):
    """Keep the per-step part of every dropout key in device memory (see above); returns the int64 scalar."""
    if _seed_state["base_dev"] is None or _seed_state["base_dev"].device != torch.device(device):
        _seed_state["base_dev"] = torch.zeros((), dtype=torch.int64, device=device)
    _write_base_dev()
    return _seed_state["base_dev"]


def disable_graph_rng():
    _seed_state["base_dev"] = None


def seed_base_ptr():
    t = _seed_state["base_dev"]
    return None if t is None else t.data_ptr()


def next_seed():
    """The by-value part of a fresh 64-bit dropout key for one call site (forward and backward share it through ctx)."""
    _seed_state["ctr"] += 1
    if _seed_state["base_dev"] is not None:
        return _seed_state["ctr"]
    return (_base_value() + _seed_state["ctr"]) & _M64


def collate_seed():
    """A fresh by-value 64-bit key for the input pipeline (MLM masking in data.device_collate).  The collate runs OUTSIDE the
    training step (and outside a captured hipGraph), before set_rng_step() of the step that will consume the batch, so it has its
    own stream: (seed, batch counter) in a key range no dropout site uses -- never the device-resident base, whose by-value part
    restarts every step (the same tokens would be masked on every replay)."""
    _seed_state["collate_ctr"] = _seed_state.get("collate_ctr", 0) + 1
    hi = (_seed_state["seed"] ^ 0xC011A7E5) & 0xFFFFFFFF
    return ((hi << 32) | (_seed_state["collate_ctr"] & 0xFFFFFFFF)) & _M64


def collate_counter():
    """Position of the collate key stream (saved in checkpoints so a resumed run does not replay the masks of batches 1..k)."""
    return int(_seed_state.get("collate_ctr", 0))


def set_collate_counter(n):
    _seed_state["collate_ctr"] = int(n)


def dropout(x, p, training):
    if not training or p <= 0.0:
        return x
    return _Dropout.apply(x, float(p), next_seed())


class _RowScaleAdd(torch.autograd.Function):
    """out = resid + scale[b] * x  (per-sample DropPath on a residual branch)."""

    @staticmethod
    def forward(ctx, resid, x, scale):
        resid, x = _c(resid), _c(x)
        out = torch.empty_like(x)
        per = x.numel() // x.shape[0]
        lib.call("fiber_rowscale_add_bf16", lib.ptr(resid), lib.ptr(x), lib.ptr(scale), lib.ptr(out), x.numel(), per)
        ctx.save_for_backward(scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        (scale,) = ctx.saved_tensors
        dout = _c(dout)
        dx = torch.empty_like(dout)
        per = dout.numel() // dout.shape[0]
        lib.call("fiber_rowscale_add_bf16", None, lib.ptr(dout), lib.ptr(scale), lib.ptr(dx), dout.numel(), per)
        return dout, dx, None


def drop_path_scale(batch, p, device):
    """timm 0.4.12 DropPath factor per sample: floor(keep + U[0,1)) / keep (fp32 [batch]), U from the path's counter-based
    key stream (csrc/elementwise.hip) -- no host generator, so the draw is capturable in a hipGraph."""
    out = torch.empty(batch, dtype=torch.float32, device=device)
    lib.call("fiber_droppath_scale_f32", lib.ptr(out), batch, 1.0 - p, next_seed(), seed_base_ptr())
    return out


def rowscale_add(resid, x, scale):
    return _RowScaleAdd.apply(resid, x, scale)


def drop_path_add(resid, x, p, training):
    """resid + DropPath_p(x): timm 0.4.12 per-sample mask floor(keep + U[0,1)) scaled by 1/keep."""
    if not training or p <= 0.0:
        return add(resid, x)
    return _RowScaleAdd.apply(resid, x, drop_path_scale(x.shape[0], p, x.device))


class _RobertaEmbed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, word, pos_tab, type_tab, gamma, beta, pad, eps, p_drop, seed):
        B, S = ids.shape
        C = word.shape[1]
        ids = _c(ids)
        word, pos_tab, type_tab, gamma, beta = (_c(t) for t in (word, pos_tab, type_tab, gamma, beta))
        y = torch.empty((B, S, C), dtype=BF16, device=ids.device)
        pos = torch.empty((B, S), dtype=torch.int32, device=ids.device)
        mean = torch.empty(B * S, dtype=torch.float32, device=ids.device)
        rstd = torch.empty_like(mean)
        lib.call("fiber_roberta_embed_fwd", lib.ptr(ids), lib.ptr(word), lib.ptr(pos_tab), lib.ptr(type_tab), lib.ptr(gamma), lib.ptr(beta),
                 lib.ptr(y), lib.ptr(pos), lib.ptr(mean), lib.ptr(rstd), B, S, C, pad, eps, p_drop, seed, seed_base_ptr())
        ctx.save_for_backward(ids, pos, word, pos_tab, type_tab, gamma, mean, rstd)
        ctx.cfg = (B, S, C, pad, p_drop, seed, seed_base_ptr())
        return y

    @staticmethod
    def backward(ctx, dy):
        ids, pos, word, pos_tab, type_tab, gamma, mean, rstd = ctx.saved_tensors
        B, S, C, pad, p_drop, seed, base = ctx.cfg
        dy = _c(dy)
        # untouched table rows stay zero; the rows present, dtype row 0, dgamma and dbeta are overwritten (fixed-order sums)
        dword, dpos, dtype = torch.zeros_like(word), torch.zeros_like(pos_tab), torch.zeros_like(type_tab)
        dg = torch.empty(C, dtype=torch.float32, device=dy.device)
        db = torch.empty_like(dg)
        ws = torch.empty(lib.plain("fiber_roberta_embed_bwd_workspace", B, S, C), dtype=torch.float32, device=dy.device)
        lib.call("fiber_roberta_embed_bwd", lib.ptr(dy), lib.ptr(ids), lib.ptr(pos), lib.ptr(word), lib.ptr(pos_tab), lib.ptr(type_tab),
                 lib.ptr(gamma), lib.ptr(mean), lib.ptr(rstd), lib.ptr(dword), lib.ptr(dpos), lib.ptr(dtype), lib.ptr(dg), lib.ptr(db),
                 lib.ptr(ws), B, S, C, pad, p_drop, seed, base)
        return None, dword, dpos, dtype, dg, db, None, None, None, None


def roberta_embed(ids, word, pos_tab, type_tab, gamma, beta, pad=1, eps=1e-5, p_drop=0.0, training=False):
    p = float(p_drop) if training else 0.0
    return _RobertaEmbed.apply(ids, word, pos_tab, type_tab, gamma, beta, pad, eps, p, next_seed() if p > 0 else 0)


class ImagePair:
    """The image batch of the one-pass MLM + ITM step, [img ; where(sel, img, alt)] (objectives.compute_mlm_itm_fused), as its two sources:
    the patch embedding gathers its im2col rows from them (fiber_im2col_patch4_pair), so neither the `where` nor the `cat` pass over the fp32
    images runs.  `tensor()` builds the batch for any other consumer."""

    def __init__(self, img, alt, sel):
        assert img.shape == alt.shape and sel.numel() == img.shape[0]
        self.img, self.alt, self.sel = img, alt, sel.reshape(-1).to(torch.bool)
        self.shape = torch.Size((2 * img.shape[0],) + tuple(img.shape[1:]))
        self.device, self.dtype, self.is_cuda = img.device, img.dtype, img.is_cuda

    def size(self, d=None):
        return self.shape if d is None else self.shape[d]

    def tensor(self):
        return torch.cat([self.img, torch.where(self.sel.view(-1, 1, 1, 1), self.img, self.alt)], 0)


def _patch_embed_weight(weight):
    """[Cout, 3, 4, 4] fp32 parameter -> bf16 [Cout, 64]: the 48 im2col columns, then zeros (the GEMM's K is a multiple of 64)."""
    key = ("pe", id(weight))
    hit = _cache_get(key, weight)
    if hit is None or hit[0] != _stamp(weight) or hit[1].device != weight.device:
        wp = torch.zeros((weight.shape[0], 64), dtype=BF16, device=weight.device)
        wp[:, :48] = weight.detach().reshape(weight.shape[0], 48).to(BF16)
        _cache_put(key, _stamp(weight), wp, weight)
    return _wcache[key][1]


class _PatchEmbedProj(torch.autograd.Function):
    """Conv2d(3->C, k=4, s=4) + bias as im2col + MFMA GEMM (no input gradient: the image is data)."""

    @staticmethod
    def forward(ctx, img, weight, bias, pair=None):
        Cout = weight.shape[0]
        if pair is not None:
            B, _, H, W = pair.shape
            rows = B * (H // 4) * (W // 4)
            a, b, sel = _c(pair.img.float()), _c(pair.alt.float()), pair.sel.to(torch.uint8)
            cols = torch.empty((rows, 64), dtype=BF16, device=a.device)
            lib.call("fiber_im2col_patch4_pair", lib.ptr(a), lib.ptr(b), lib.ptr(sel), lib.ptr(cols), B // 2, H, W)
            img = a
        else:
            B, _, H, W = img.shape
            img = _c(img.float())
            rows = B * (H // 4) * (W // 4)
            cols = torch.empty((rows, 64), dtype=BF16, device=img.device)
            lib.call("fiber_im2col_patch4", lib.ptr(img), lib.ptr(cols), B, H, W)
        y, _ = gemm_nt(cols, _patch_embed_weight(weight), bias)
        ctx.save_for_backward(cols)
        ctx.wshape = weight.shape
        return y.view(B, rows // B, Cout)

    @staticmethod
    def backward(ctx, dy):
        (cols,) = ctx.saved_tensors
        dy2 = _c(dy).view(-1, dy.shape[-1])
        w_, db = wgrad(dy2, cols, want_bias=True)
        dw = torch.empty(ctx.wshape, dtype=w_.dtype, device=w_.device)    # a fresh tensor, not a view of a temporary: autograd takes it over as .grad
        dw.view(w_.shape[0], 48).copy_(w_[:, :48])
        return None, dw, db, None


def patch_embed_proj(img, weight, bias):
    if isinstance(img, ImagePair):
        if img.is_cuda:
            return _PatchEmbedProj.apply(None, weight, bias, img)
        img = img.tensor()
    return _PatchEmbedProj.apply(img, weight, bias)


# ---------------------------------------------------------------------------------------------------------------------------
# Modulated deformable convolution (DyHead of the fine-grained model): csrc/dcn.hip gather / scatter around the
# hand-written NT / TN GEMMs.  Channels-last throughout.
def _conv_weight_rows(weight, transposed=False):
    """[Cout, Cin, kh, kw] fp32 parameter -> bf16 [Cp, kh*kw*Cin] in the tap-major column order of the gather kernel (rows padded
    with zeros to a multiple of 8 -- the 27-channel offset convolution), or its transpose [kh*kw*Cin, Cp] for the dgrad GEMM."""
    key = ("KCT" if transposed else "KC", id(weight))
    hit = _cache_get(key, weight)
    if hit is not None and hit[0] == _stamp(weight) and hit[1].device == weight.device:
        return hit[1]
    if transposed:
        v = _conv_weight_rows(weight).t().contiguous()
    else:
        Cout = weight.shape[0]
        v = weight.detach().permute(0, 2, 3, 1).reshape(Cout, -1).to(BF16)
        if Cout % 8:
            v = torch.nn.functional.pad(v, (0, 0, 0, 8 - Cout % 8))
        v = v.contiguous()
    _cache_put(key, _stamp(weight), v, weight)
    return v


def _conv_out(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


class _DeformConv(torch.autograd.Function):
    """y[B,Ho,Wo,Cout] = conv(x[B,H,W,Cin] sampled at taps + offset, * mask) + bias.  offset [M, 2*taps] / mask [M, taps] fp32 or
    None (ordinary convolution).  Forward: one gather launch + one MFMA GEMM over the whole batch; backward: dgrad GEMM -> one
    scatter launch (dx, doffset, dmask), weight + bias gradient on the TN kernel."""

    @staticmethod
    def forward(ctx, x, offset, mask, weight, bias, stride, pad, out_fp32=False):
        B, H, W, C = x.shape
        Cout, _, kh, kw = weight.shape
        Ho, Wo = _conv_out(H, kh, stride, pad), _conv_out(W, kw, stride, pad)
        x = _c(x)
        offset = _c(offset.float()) if offset is not None else None
        mask = _c(mask.float()) if mask is not None else None
        M = B * Ho * Wo
        cols = torch.empty((M, kh * kw * C), dtype=BF16, device=x.device)
        lib.call("fiber_dcn_gather_bf16", lib.ptr(x), lib.ptr(offset), lib.ptr(mask), lib.ptr(cols), B, H, W, C, Ho, Wo, kh, kw, stride, pad)
        wr = _conv_weight_rows(weight)
        Cp = wr.shape[0]
        bp = bias
        if bias is not None and Cp != Cout:
            bp = torch.nn.functional.pad(bias.detach().float(), (0, Cp - Cout))
        y, _ = gemm_nt(cols, wr, bp, out_fp32=out_fp32)
        if Cp != Cout:
            y = y[:, :Cout].contiguous()
        ctx.save_for_backward(x, offset, mask, cols, weight)
        ctx.geom = (B, H, W, C, Ho, Wo, kh, kw, stride, pad, Cout, Cp)
        ctx.has_bias = bias is not None
        return y.view(B, Ho, Wo, Cout)

    @staticmethod
    def backward(ctx, dy):
        x, offset, mask, cols, weight = ctx.saved_tensors
        B, H, W, C, Ho, Wo, kh, kw, stride, pad, Cout, Cp = ctx.geom
        dy2 = _c(dy.to(BF16)).view(-1, Cout)
        if Cp != Cout:
            dy2 = torch.nn.functional.pad(dy2, (0, Cp - Cout))
        dx = doff = dmask = dw = db = None
        need_x, need_off, need_mask = ctx.needs_input_grad[0], offset is not None and ctx.needs_input_grad[1], mask is not None and ctx.needs_input_grad[2]
        if need_x or need_off or need_mask:
            dcols, _ = gemm_nt(dy2, _conv_weight_rows(weight, transposed=True))
            tiled = need_x and kh == 3 and kw == 3 and pad == 1 and stride in (1, 2) and C % 16 == 0      # atomics-free input gradient
            dxf = torch.zeros((B, H, W, C), dtype=torch.float32, device=x.device) if (need_x and not tiled) else None
            doff = torch.empty_like(offset) if need_off else None
            dmask = torch.empty_like(mask) if need_mask else None
            if dxf is not None or need_off or need_mask:
                lib.call("fiber_dcn_scatter_bf16", lib.ptr(dcols), lib.ptr(x), lib.ptr(offset), lib.ptr(mask), lib.ptr(dxf), lib.ptr(doff),
                         lib.ptr(dmask), B, H, W, C, Ho, Wo, kh, kw, stride, pad)
            if tiled:
                n = lib.plain("fiber_dcn_dx_workspace", B, H, W, C, Ho, Wo, stride)
                ws = torch.empty(n, dtype=torch.float32, device=x.device)
                ws[n - B * H * W * C - 4:].zero_()
                dx = torch.empty((B, H, W, C), dtype=BF16, device=x.device)
                lib.call("fiber_dcn_dx_bf16", lib.ptr(dcols), lib.ptr(offset), lib.ptr(mask), lib.ptr(dx), lib.ptr(ws), B, H, W, C, Ho, Wo,
                         kh, kw, stride, pad)
            elif need_x:
                dx = dxf.to(BF16)
        need_db = ctx.has_bias and ctx.needs_input_grad[4]
        if ctx.needs_input_grad[3]:
            w_, b_ = wgrad(dy2, cols, want_bias=True) if need_db else (wgrad(dy2, cols), None)
            dw, db = w_[:Cout].view(Cout, kh, kw, C).permute(0, 3, 1, 2).contiguous(), b_[:Cout] if b_ is not None else None
        elif need_db:
            db = colsum(dy2)[:Cout]
        return dx, doff, dmask, dw, db, None, None, None


def deform_conv(x, offset, mask, weight, bias=None, stride=1, pad=1, out_fp32=False):
    """Channels-last modulated deformable convolution; offset = mask = None gives the ordinary convolution.  out_fp32: the result
    is stored in fp32 (the offset / mask predictor: the reference runs the whole operator in fp32, deform_conv.py:335, and sampling
    positions rounded to bf16 move every bilinear weight by up to 2^-9 of the offset)."""
    return _DeformConv.apply(x, offset, mask, weight, bias, stride, pad, out_fp32)


# ---- grounding head: region-word alignment + binary token focal loss (csrc/ground.hip) ---------------------------------------------
def _ground_inputs(x, p, tbias, log_scale):
    B, A, C = x.shape
    T = p.shape[1]
    if p.shape != (B, T, C) or tbias.shape != (B, T) or log_scale.numel() != 1:
        raise ValueError(f"ground: x {tuple(x.shape)}, p {tuple(p.shape)}, tbias {tuple(tbias.shape)}, log_scale {tuple(log_scale.shape)}")
    return (_c(x.detach().to(BF16)), _c(p.detach().to(BF16)), _c(tbias.detach().float()), _c(log_scale.detach().float().reshape(1)),
            B, A, T, C)


def _ground_workspace(B, A, T, device):
    return torch.empty(max(1, lib.plain("fiber_ground_workspace", B, A, T)), dtype=torch.float32, device=device)


def _ground_operand_grads(ctx, ds, x16, p16):
    """dX = ds . P (NT kernel) and dP = ds^T . X (TN kernel), image by image: P differs per image."""
    B, A, T = ds.shape
    dx = dp = None
    if ctx.needs_input_grad[0]:
        pt = p16.transpose(1, 2).contiguous()                      # [B, C, T]: the W operand of Y = X . W^T
        dx = torch.empty((B, A, pt.shape[1]), dtype=BF16, device=ds.device)
        for b in range(B):                                         # written in place: no second [B, A, C] copy at the full geometry
            lib.call("fiber_gemm_nt_bf16", lib.ptr(ds[b]), lib.ptr(pt[b]), None, None, lib.ptr(dx[b]), None, None, 0, None, 0, None,
                     A, pt.shape[1], T, T, T, pt.shape[1], 0, 0)
    if ctx.needs_input_grad[1]:
        # dP is an ACTIVATION gradient (it flows on into the text projection); P differs per image, so the TN kernel is called image by image
        C = x16.shape[2]
        dp = torch.empty((B, T, C), dtype=torch.float32, device=ds.device)
        S = lib.plain("fiber_gemm_tn_splits", A, T, C)
        ws = torch.empty(S * (T * C + T), dtype=torch.float32, device=ds.device) if S > 1 else None
        for b in range(B):
            lib.call("fiber_gemm_tn_bf16", lib.ptr(ds[b]), lib.ptr(x16[b]), lib.ptr(dp[b]), None, lib.ptr(ws), A, T, C, T, C, None, 0, 1.0)
    return dx, dp


class _GroundLogits(torch.autograd.Function):
    """The plain path: s materialised in fp32.  Backward: ds = dlogits where the clamp is inactive, as bf16, through the same two
    GEMMs as the fused path."""

    @staticmethod
    def forward(ctx, x, p, tbias, log_scale):
        x16, p16, tb, ls, B, A, T, C = _ground_inputs(x, p, tbias, log_scale)
        out = torch.empty((B, A, T), dtype=torch.float32, device=x.device)
        lib.call("fiber_ground_fwd_bf16", lib.ptr(x16), lib.ptr(p16), lib.ptr(tb), lib.ptr(ls), None, None, lib.ptr(out), None, None,
                 B, A, T, C, -1.0, 0.0)
        ctx.save_for_backward(x16, p16, tb, ls, out)
        ctx.dtypes = (x.dtype, p.dtype, tbias.dtype, log_scale.dtype, log_scale.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        x16, p16, tb, ls, out = ctx.saved_tensors
        inv = torch.exp(-ls)
        dsf = torch.where(out.abs() < 50000.0, dout.float(), torch.zeros((), device=out.device))     # clamp inactive
        dtb = dsf.sum(1) if ctx.needs_input_grad[2] else None
        dls = -(dsf * (out - tb[:, None, :])).sum().reshape(ctx.dtypes[4]) if ctx.needs_input_grad[3] else None
        dx, dp = _ground_operand_grads(ctx, (dsf * inv).to(BF16), x16, p16)
        return (dx.to(ctx.dtypes[0]) if dx is not None else None, dp.to(ctx.dtypes[1]) if dp is not None else None,
                dtb.to(ctx.dtypes[2]) if dtb is not None else None, dls.to(ctx.dtypes[3]) if dls is not None else None)


class _GroundTokenLoss(torch.autograd.Function):
    """The fused path: forward = one launch that writes a scalar; backward = one launch that recomputes the tile and emits ds
    (bf16) + the dtbias / dlog_scale sums, then the two GEMMs.  Nothing of size [B, A, T] is saved."""

    @staticmethod
    def forward(ctx, x, p, tbias, log_scale, targets, text_mask, alpha, gamma):
        x16, p16, tb, ls, B, A, T, C = _ground_inputs(x, p, tbias, log_scale)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        ws = _ground_workspace(B, A, T, x.device)
        lib.call("fiber_ground_fwd_bf16", lib.ptr(x16), lib.ptr(p16), lib.ptr(tb), lib.ptr(ls), lib.ptr(targets), lib.ptr(text_mask), None,
                 lib.ptr(loss), lib.ptr(ws), B, A, T, C, float(alpha), float(gamma))
        ctx.save_for_backward(x16, p16, tb, ls, targets, text_mask)
        ctx.hyper = (float(alpha), float(gamma))
        ctx.dtypes = (x.dtype, p.dtype, tbias.dtype, log_scale.dtype, log_scale.shape)
        return loss

    @staticmethod
    def backward(ctx, g):
        x16, p16, tb, ls, targets, text_mask = ctx.saved_tensors
        B, A, C = x16.shape
        T = p16.shape[1]
        dev = x16.device
        ds = torch.empty((B, A, T), dtype=BF16, device=dev)
        dtb = torch.empty((B, T), dtype=torch.float32, device=dev)
        dls = torch.empty(1, dtype=torch.float32, device=dev)
        ws = _ground_workspace(B, A, T, dev)
        g32 = _c(g.detach().float().reshape(1))
        lib.call("fiber_ground_bwd_bf16", lib.ptr(x16), lib.ptr(p16), lib.ptr(tb), lib.ptr(ls), lib.ptr(targets), lib.ptr(text_mask),
                 lib.ptr(g32), lib.ptr(ds), lib.ptr(dtb), lib.ptr(dls), lib.ptr(ws), B, A, T, C, *ctx.hyper)
        dx, dp = _ground_operand_grads(ctx, ds, x16, p16)
        return (dx.to(ctx.dtypes[0]) if dx is not None else None, dp.to(ctx.dtypes[1]) if dp is not None else None,
                dtb.to(ctx.dtypes[2]) if ctx.needs_input_grad[2] else None,
                dls.reshape(ctx.dtypes[4]).to(ctx.dtypes[3]) if ctx.needs_input_grad[3] else None, None, None, None, None)


def ground_logits(x, p, tbias, log_scale):
    """fp32 [B, A, T] alignment logits clamp(x . p^T * exp(-log_scale) + tbias, +-50000) (vldyhead.py:857-891); x [B, A, 256] tower
    features (rounded to bf16), p [B, 256, 256] projected tokens (rounded to bf16), tbias fp32 [B, 256], log_scale one element."""
    return _GroundLogits.apply(x, p, tbias, log_scale)


def ground_token_loss(x, p, tbias, log_scale, targets, text_mask=None, alpha=0.25, gamma=2.0):
    """Sum over anchors and unmasked tokens of the binary token focal loss of the alignment logits (sigmoid_focal_loss.py:130-195,
    TokenSigmoidFocalLoss version="binary"), without materialising them.  targets [B, A, T] holding 0/1 in any dtype (converted to
    uint8 once); text_mask [B, T] (> 0 = live) or None = all tokens."""
    if targets.numel() == 0:
        return torch.zeros((), dtype=torch.float32, device=x.device)
    if targets.shape != (x.shape[0], x.shape[1], p.shape[1]):
        raise ValueError(f"ground_token_loss: targets {tuple(targets.shape)} for x {tuple(x.shape)}, p {tuple(p.shape)}")
    t8 = _c(targets if targets.dtype == torch.uint8 else (targets != 0).to(torch.uint8))
    m8 = torch.ones(p.shape[:2], dtype=torch.uint8, device=x.device) if text_mask is None else _c((text_mask > 0).to(torch.uint8))
    return _GroundTokenLoss.apply(x, p, tbias, log_scale, t8, m8, alpha, gamma)


# ---- grounding inference: scores, decode, multi-label NMS (csrc/detect.hip); inference only, no autograd ----------------------------
def _det_f32(t):
    return _c(t.detach().float())


def det_scores(logits, centerness, class_ptr, tok_idx, pre_nms_thresh, score_agg="MEAN"):
    """Dense class scores of one level (inference.py:620-650, :741-795): logits fp32 [B, A, 256] and centerness [B, 1, H, W] as
    VLDyHead.forward returns them, the positive map as CSR (int32 class_ptr [C + 1], tok_idx [nnz]), or one map per sample as class_ptr
    [B, C + 1] holding absolute offsets into the one tok_idx (grounding_inference.pack_positive_maps).  -> fp32 [B, A, C]:
    agg * sigmoid(centerness) where agg > pre_nms_thresh, -1 elsewhere."""
    if score_agg not in ("MEAN", "MAX"):
        raise NotImplementedError(f"det_scores: score_agg {score_agg!r} (MEAN and MAX are built)")
    B, A, T = logits.shape
    C = class_ptr.shape[-1] - 1
    if centerness.numel() != B * A or class_ptr.dtype != torch.int32 or tok_idx.dtype != torch.int32:
        raise ValueError(f"det_scores: logits {tuple(logits.shape)}, centerness {tuple(centerness.shape)}, CSR {class_ptr.dtype} / {tok_idx.dtype}")
    lg, ct = _det_f32(logits), _det_f32(centerness)
    out = torch.empty((B, A, C), dtype=torch.float32, device=logits.device)
    if class_ptr.dim() == 1:
        lib.call("fiber_det_scores_f32", lib.ptr(lg), lib.ptr(ct), lib.ptr(_c(class_ptr)), lib.ptr(_c(tok_idx)), lib.ptr(out), B, A, T, C,
                 float(pre_nms_thresh), int(score_agg == "MAX"))
        return out
    if class_ptr.dim() != 2 or class_ptr.shape[0] != B:
        raise ValueError(f"det_scores: class_ptr {tuple(class_ptr.shape)} for {B} samples (one row of C + 1 offsets per sample)")
    lib.call("fiber_det_scores_rows_f32", lib.ptr(lg), lib.ptr(ct), lib.ptr(_c(class_ptr)), lib.ptr(_c(tok_idx)), lib.ptr(out), B, A, T, C,
             float(pre_nms_thresh), int(score_agg == "MAX"), C + 1)
    return out


def det_decode(topk_val, topk_idx, bbox_reg, anchors, image_sizes, out, offset, level, num_classes, min_size=0.0):
    """Decode one level's top-k into the slice [offset, offset + k) of the concatenated buffers out = (boxes [B, N, 4] fp32, scores
    [B, N] fp32, labels [B, N] int32, source [B, N] int32) in place (inference.py:657-676, box_coder.py:52-95, clip_to_image,
    remove_small_boxes).  bbox_reg fp32 [B, 4, H, W] is read in place; anchors [H * W, 4]; image_sizes fp32 [B, 2] as (w, h)."""
    boxes, scores, labels, source = out
    B, k = topk_val.shape
    A = anchors.shape[0]
    N = scores.shape[1]
    if bbox_reg.shape[0] != B or bbox_reg.numel() != B * 4 * A or topk_idx.dtype != torch.int64 or image_sizes.shape != (B, 2):
        raise ValueError(f"det_decode: bbox_reg {tuple(bbox_reg.shape)} for {A} anchors, topk_idx {topk_idx.dtype}, sizes {tuple(image_sizes.shape)}")
    for t, dt in ((boxes, torch.float32), (scores, torch.float32), (labels, torch.int32), (source, torch.int32)):
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError("det_decode: the output buffers are contiguous fp32 / fp32 / int32 / int32")
    lib.call("fiber_det_decode_f32", lib.ptr(_det_f32(topk_val)), lib.ptr(_c(topk_idx)), lib.ptr(_det_f32(bbox_reg)),
             lib.ptr(_det_f32(anchors)), lib.ptr(_det_f32(image_sizes)), lib.ptr(boxes), lib.ptr(scores), lib.ptr(labels), lib.ptr(source),
             B, k, A, int(num_classes), N, int(offset), int(level), float(min_size))


def nms_ml(boxes, scores, labels, source, nms_thresh, detections_per_img):
    """Multi-label NMS of candidates ALREADY SORTED by descending score per image (ml_nms.cu; padding = score < 0 at the end) and the
    cut to detections_per_img (select_over_all_levels).  boxes [B, N, 4], scores [B, N] fp32, labels / source [B, N] int32.
    -> (boxes [B, D, 4], scores [B, D], labels [B, D], source [B, D], count [B]); no host synchronisation."""
    B, N = scores.shape
    D = int(detections_per_img)
    dev = scores.device
    if B == 0 or N == 0:                                     # no launch: the padding the select kernel would have written
        return (torch.zeros((B, D, 4), dtype=torch.float32, device=dev), torch.full((B, D), -1.0, dtype=torch.float32, device=dev),
                torch.zeros((B, D), dtype=torch.int32, device=dev), torch.full((B, D), -1, dtype=torch.int32, device=dev),
                torch.zeros((B,), dtype=torch.int32, device=dev))
    ob = torch.empty((B, D, 4), dtype=torch.float32, device=dev)   # the select kernel writes every element, past count included
    osc = torch.empty((B, D), dtype=torch.float32, device=dev)
    ol, osr = torch.empty((B, D), dtype=torch.int32, device=dev), torch.empty((B, D), dtype=torch.int32, device=dev)
    cnt = torch.empty((B,), dtype=torch.int32, device=dev)
    bx, sc = _det_f32(boxes), _det_f32(scores)
    lb, sr = _c(labels.to(torch.int32)), _c(source.to(torch.int32))
    mask = torch.empty((B, N, (N + 63) // 64), dtype=torch.int64, device=dev)
    lib.call("fiber_det_nms_mask", lib.ptr(bx), lib.ptr(sc), lib.ptr(lb), lib.ptr(mask), B, N, float(nms_thresh))
    lib.call("fiber_det_nms_select", lib.ptr(bx), lib.ptr(sc), lib.ptr(lb), lib.ptr(sr), lib.ptr(mask), lib.ptr(ob), lib.ptr(osc),
             lib.ptr(ol), lib.ptr(osr), lib.ptr(cnt), B, N, D)
    return ob, osc, ol, osr, cnt


def det_merge_max_candidates():
    return int(lib.plain("fiber_det_merge_max_candidates"))


DET_MERGE_MAX_CHUNKS, DET_MERGE_MAX_CANDIDATES = 64, 16384   # = det_merge_max_candidates(); the host path keeps the same bounds


def _det_merge_host(boxes, scores, labels, source, count, label_table, N, out):
    """fiber_det_merge on CPU tensors, in numpy (a stable sort of the live slots in chunk order, then slot order)"""
    import numpy as np
    bx, sc, lb, sr = boxes.detach().float().numpy(), scores.detach().float().numpy(), labels.numpy(), source.numpy()
    cnt, tab = count.numpy(), label_table.numpy()
    B, K, D = sc.shape
    Cc = tab.shape[1]
    ob, osc, ol, osr, och, ocnt = (t.numpy() for t in out)
    ob[:], osc[:], ol[:], osr[:], och[:] = 0.0, -1.0, 0, -1, -1
    for b in range(B):
        live = np.arange(D)[None, :] < np.clip(cnt[b], 0, D)[:, None]
        k, s = np.nonzero(live)                              # row-major: chunk order, then slot order
        order = np.argsort(-sc[b, k, s].astype(np.float64), kind="stable")[:N]
        k, s, n = k[order], s[order], len(order)
        local = lb[b, k, s]
        ok = (local >= 1) & (local <= Cc)
        ob[b, :n], osc[b, :n], osr[b, :n], och[b, :n] = bx[b, k, s], sc[b, k, s], sr[b, k, s], k
        ol[b, :n] = np.where(ok, tab[k, np.clip(local - 1, 0, Cc - 1)], 0) if Cc else 0
        ocnt[b] = n
    return out


def det_merge(boxes, scores, labels, source, count, label_table, max_dets=None, out=None):
    """Merge the K per-chunk results of each image into one ranked list (chunked open-vocabulary detection; lvis_eval.py:137-148's
    sorted(.., reverse=True)[:max_dets] over the concatenation).  boxes fp32 [B, K, D, 4], scores fp32 [B, K, D], labels / source int32
    [B, K, D], count int32 [B, K], label_table int32 [K, Cc] (chunk-local class -> output label).  CONTRACT: the first count[b, k] scores
    of every (b, k) descend, which is how Detections come; the slots past count are ignored whatever they hold.
    -> (boxes [B, N, 4], scores [B, N], labels [B, N], source [B, N], chunk [B, N], count [B]), N = K * D, or min(max_dets, K * D):
    descending score, equal scores to the earlier chunk, then the earlier slot; labels = label_table[k, local - 1] (0 for a local label
    outside 1..Cc), source unchanged, chunk = k; past count the padding of nms_ml and chunk -1.  One launch, no synchronisation; on CPU
    tensors the same in numpy.  out: the six result tensors to write into (contiguous, of the result's shapes and dtypes)."""
    if boxes.dim() != 4 or scores.dim() != 3:
        raise ValueError(f"det_merge: boxes {tuple(boxes.shape)}, scores {tuple(scores.shape)}: [B, K, D, 4] and [B, K, D]")
    B, K, D = scores.shape
    if boxes.shape != (B, K, D, 4) or labels.shape != (B, K, D) or source.shape != (B, K, D) or count.shape != (B, K) or \
            label_table.dim() != 2 or label_table.shape[0] != K:
        raise ValueError(f"det_merge: boxes {tuple(boxes.shape)}, labels {tuple(labels.shape)}, source {tuple(source.shape)}, count "
                         f"{tuple(count.shape)}, label_table {tuple(label_table.shape)} for scores {tuple(scores.shape)}")
    if boxes.dtype != torch.float32 or scores.dtype != torch.float32 or labels.dtype != torch.int32 or source.dtype != torch.int32 or \
            count.dtype != torch.int32 or label_table.dtype != torch.int32:
        raise ValueError("det_merge: boxes / scores fp32, labels / source / count / label_table int32")
    if K > DET_MERGE_MAX_CHUNKS or K * D > DET_MERGE_MAX_CANDIDATES:
        raise ValueError(f"det_merge: {K} chunks x {D} slots exceed the merge kernel's capacity of {DET_MERGE_MAX_CHUNKS} chunks and "
                         f"{DET_MERGE_MAX_CANDIDATES} candidates per image")
    if max_dets is not None and int(max_dets) < 0:
        raise ValueError(f"det_merge: max_dets {max_dets}")
    dev = scores.device
    if any(t.device != dev for t in (boxes, labels, source, count, label_table)):
        raise ValueError("det_merge: the tensors lie on different devices")
    N = K * D if max_dets is None else min(int(max_dets), K * D)
    shapes = (((B, N, 4), torch.float32), ((B, N), torch.float32), ((B, N), torch.int32), ((B, N), torch.int32), ((B, N), torch.int32),
              ((B,), torch.int32))
    if out is None:
        out = tuple(torch.empty(s, dtype=dt, device=dev) for s, dt in shapes)      # the kernel writes every element
    elif len(out) != 6 or any(t.shape != s or t.dtype != dt or t.device != dev or not t.is_contiguous() for t, (s, dt) in zip(out, shapes)):
        raise ValueError(f"det_merge: out must be six contiguous tensors on {dev} of {shapes}")
    if B == 0 or N == 0:                                     # nothing to rank: no launch
        out[5].zero_()
        return tuple(out)
    if not scores.is_cuda:
        return tuple(_det_merge_host(boxes, scores, labels, source, count, label_table, N, out))
    ob, osc, ol, osr, och, ocnt = out
    lib.call("fiber_det_merge", lib.ptr(_c(boxes)), lib.ptr(_c(scores)), lib.ptr(_c(labels)), lib.ptr(_c(source)), lib.ptr(_c(count)),
             lib.ptr(_c(label_table)), lib.ptr(ob), lib.ptr(osc), lib.ptr(ol), lib.ptr(osr), lib.ptr(och), lib.ptr(ocnt), B, K, D,
             int(label_table.shape[1]), N)
    return ob, osc, ol, osr, och, ocnt


# ---- multi-scale test-time augmentation: collect the views' candidates, merge them class by class (csrc/detect.hip) -----------------
DET_AUG_MAX_CANDIDATES = 1 << 20                             # = det_aug_max_candidates(); the host path keeps the same bound
DET_AUG_MODES = {"none": 0, "vote": 1}
_DET_AUG_DEAD = 1 << 30                                      # the label dead slots sort under (AUG_DEAD_LABEL)


def det_aug_max_candidates():
    return int(lib.plain("fiber_det_aug_max_candidates"))


def _det_aug_view_dtype():
    import numpy as np
    return np.dtype([("scaled_w", "<f4"), ("ratio_w", "<f4"), ("ratio_h", "<f4"), ("equal", "<i4"), ("flip", "<i4"), ("has_range", "<i4"),
                     ("min2", "<f4"), ("max2", "<f4")])


def det_aug_view_rows(originals, sizes, flip, keep_range=None):
    """The per-image records of one view for det_aug_collect.  originals: (H, W) per image, sizes: (oh, ow) of the resized images (the
    frame the view's candidates are in), flip: the view ran on the mirrored images, keep_range: TEST.RANGES' (min, max) or None.
    The ratios are BoxList.resize's (bounding_box.py:110): computed in double, compared in double, applied as fp32."""
    rows = []
    for (H, W), (oh, ow) in zip(originals, sizes):
        rw, rh = float(W) / float(ow), float(H) / float(oh)
        lo, hi = (0.0, 0.0) if keep_range is None else (float(keep_range[0] * keep_range[0]), float(keep_range[1] * keep_range[1]))
        rows.append((float(ow), rw, rh, int(rw == rh), int(bool(flip)), int(keep_range is not None), lo, hi))
    return rows


def _det_aug_check_classes(classes, dev, what):
    if classes.dim() != 1 or classes.dtype != torch.int32 or classes.device != dev:
        raise ValueError(f"{what}: classes {tuple(classes.shape)} {classes.dtype} on {classes.device}: an ascending int32 [C] table on {dev}")


def _det_aug_collect_host(boxes, scores, labels, source, table, classes, out, offset, view):
    """fiber_det_aug_collect on CPU tensors, in numpy (fp32 throughout, the kernel's operation order)"""
    import numpy as np
    bx, sc, lb, sr = boxes.detach().float().numpy(), scores.detach().float().numpy(), labels.numpy(), source.numpy()
    ob, osc, ol, osr, ov = (t.numpy() for t in out)
    Nv = sc.shape[1]
    one = np.float32(1)
    for b, p in enumerate(table):
        x1, y1, x2, y2 = (bx[b, :, i].copy() for i in range(4))
        live = (sc[b] >= 0) & np.isin(lb[b], classes.numpy())
        if p["flip"]:
            x1, x2 = p["scaled_w"] - x2 - one, p["scaled_w"] - x1 - one
        if p["has_range"]:
            area = (x2 - x1 + one) * (y2 - y1 + one)
            live &= (area > p["min2"]) & (area < p["max2"])
        ry = p["ratio_w"] if p["equal"] else p["ratio_h"]
        box = np.stack((x1 * p["ratio_w"], y1 * ry, x2 * p["ratio_w"], y2 * ry), axis=1).astype(np.float32)
        at = slice(offset, offset + Nv)
        ob[b, at] = np.where(live[:, None], box, np.float32(0))
        osc[b, at], ol[b, at] = np.where(live, sc[b], np.float32(-1)), np.where(live, lb[b], 0)
        osr[b, at], ov[b, at] = np.where(live, sr[b], -1), np.where(live, view, -1)


def det_aug_collect(boxes, scores, labels, source, rows, classes, out, offset, view):
    """One view's candidates (ATSSPostProcessor.candidates: boxes fp32 [B, Nv, 4] in the view's resized frame, scores fp32 [B, Nv] with
    -1 padding, labels / source int32 [B, Nv]) -> the slots [offset, offset + Nv) of out = (boxes [B, T, 4], scores, labels, source, view
    [B, T]) in place: un-flipped, range-filtered in the resized frame, resized to the original frame (box_aug.py: im_detect_bbox_hflip,
    remove_boxes, add_preds_t).  rows: det_aug_view_rows(...) (host); classes: ascending int32 [C], labels outside it are dropped.
    Dropped and padding slots get box 0, score -1, label 0, source -1, view -1.  One launch, no synchronisation; on CPU tensors numpy."""
    import numpy as np
    if boxes.dim() != 3 or scores.dim() != 2:
        raise ValueError(f"det_aug_collect: boxes {tuple(boxes.shape)}, scores {tuple(scores.shape)}: [B, Nv, 4] and [B, Nv]")
    B, Nv = scores.shape
    if boxes.shape != (B, Nv, 4) or labels.shape != (B, Nv) or source.shape != (B, Nv) or len(rows) != B:
        raise ValueError(f"det_aug_collect: boxes {tuple(boxes.shape)}, labels {tuple(labels.shape)}, source {tuple(source.shape)}, "
                         f"{len(rows)} rows for scores {tuple(scores.shape)}")
    if boxes.dtype != torch.float32 or scores.dtype != torch.float32 or labels.dtype != torch.int32 or source.dtype != torch.int32:
        raise ValueError("det_aug_collect: boxes / scores fp32, labels / source int32")
    dev = scores.device
    _det_aug_check_classes(classes, dev, "det_aug_collect")
    if len(out) != 5:
        raise ValueError("det_aug_collect: out is (boxes, scores, labels, source, view)")
    T = int(out[1].shape[1]) if out[1].dim() == 2 else -1
    shapes = (((B, T, 4), torch.float32), ((B, T), torch.float32), ((B, T), torch.int32), ((B, T), torch.int32), ((B, T), torch.int32))
    if any(t.shape != s or t.dtype != dt or t.device != dev or not t.is_contiguous() for t, (s, dt) in zip(out, shapes)):
        raise ValueError(f"det_aug_collect: out must be five contiguous tensors on {dev} of {shapes}")
    if any(t.device != dev for t in (boxes, labels, source)):
        raise ValueError("det_aug_collect: the tensors lie on different devices")
    offset, view = int(offset), int(view)
    if T > DET_AUG_MAX_CANDIDATES or offset < 0 or offset + Nv > T or view < 0:
        raise ValueError(f"det_aug_collect: slots [{offset}, {offset + Nv}) of view {view} in buffers of {T} (capacity "
                         f"{DET_AUG_MAX_CANDIDATES} candidates per image)")
    table = np.zeros(B, _det_aug_view_dtype())
    for i, r in enumerate(rows):
        table[i] = tuple(r)
    if B == 0 or Nv == 0:
        return out
    if not scores.is_cuda:
        _det_aug_collect_host(boxes, scores, labels, source, table, classes, out, offset, view)
        return out
    d_table = torch.from_numpy(table.view(np.uint8).copy()).to(dev, non_blocking=True)
    lib.call("fiber_det_aug_collect", lib.ptr(_c(boxes)), lib.ptr(_c(scores)), lib.ptr(_c(labels)), lib.ptr(_c(source)), lib.ptr(d_table),
             lib.ptr(_c(classes)), *(lib.ptr(t) for t in out), B, Nv, T, offset, view, int(classes.numel()))
    return out


def _det_aug_iou(a, c):
    """IoU of box a [4] with boxes c [n, 4], fp32, +1 widths, nms.cu's operation order"""
    import numpy as np
    one, zero = np.float32(1), np.float32(0)
    w = np.maximum(np.minimum(a[2], c[:, 2]) - np.maximum(a[0], c[:, 0]) + one, zero)
    h = np.maximum(np.minimum(a[3], c[:, 3]) - np.maximum(a[1], c[:, 1]) + one, zero)
    inter = w * h
    sa = (a[2] - a[0] + one) * (a[3] - a[1] + one)
    sb = (c[:, 2] - c[:, 0] + one) * (c[:, 3] - c[:, 1] + one)
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (sa + sb - inter)


def _det_aug_merge_host(boxes, scores, labels, source, view, classes, thresh, mode, D):
    """det_aug_merge on CPU tensors, in numpy: per image and class the leader loop of the kernel, then the cut"""
    import numpy as np
    bx, sc, lb = boxes.detach().float().numpy(), scores.detach().float().numpy(), labels.numpy()
    sr, vw, cls = source.numpy(), view.numpy(), classes.numpy()
    B, T = sc.shape
    ob, osc = np.zeros((B, D, 4), np.float32), np.full((B, D), -1, np.float32)
    ol, osr, ov, cnt = np.zeros((B, D), np.int32), np.full((B, D), -1, np.int32), np.full((B, D), -1, np.int32), np.zeros(B, np.int32)
    th = np.float32(thresh)
    for b in range(B):
        live = np.nonzero((sc[b] >= 0) & np.isin(lb[b], cls))[0]
        kept_slot, kept_box = [], []
        for c in np.unique(lb[b, live]):
            seg = live[lb[b, live] == c]
            seg = seg[np.argsort(-sc[b, seg].astype(np.float64), kind="stable")]          # score descending, then slot ascending
            while len(seg):
                lead, c_box = seg[0], bx[b, seg]
                if not thresh > 0:
                    hit = np.zeros(len(seg), bool)
                else:
                    iou = _det_aug_iou(bx[b, lead], c_box)
                    hit = iou >= th if mode else iou > th
                hit[0] = True
                box = bx[b, lead]
                if mode and hit.sum() > 1:
                    s = sc[b, seg[hit]]
                    box = (c_box[hit] * s[:, None]).sum(axis=0, dtype=np.float32) / s.sum(dtype=np.float32)
                kept_slot.append(lead), kept_box.append(box)
                seg = seg[~hit]
        if not kept_slot:
            continue
        slot, kb = np.array(kept_slot), np.stack(kept_box).astype(np.float32)
        order = np.lexsort((slot, lb[b, slot], -sc[b, slot].astype(np.float64)))[:D]       # score descending, label, slot
        n = len(order)
        s = slot[order]
        ob[b, :n], osc[b, :n], ol[b, :n], osr[b, :n], ov[b, :n], cnt[b] = kb[order], sc[b, s], lb[b, s], sr[b, s], vw[b, s], n
    return tuple(torch.from_numpy(x) for x in (ob, osc, ol, osr, ov, cnt))


def det_aug_merge(boxes, scores, labels, source, view, classes, thresh, mode, top_n):
    """merge_result_from_multi_scales (box_aug.py:175-214) of each image's concatenated candidates as det_aug_collect leaves them: boxes
    fp32 [B, T, 4], scores fp32 [B, T] (< 0 = dead slot), labels / source / view int32 [B, T]; classes: ASCENDING int32 [C] WITHOUT
    repeats (TEST.SELECT_CLASSES, or 1 .. NUM_CLASSES - 1), candidates of other labels are dropped.  Per class boxlist_nms(thresh,
    nms_type=mode): "none" = greedy NMS, suppress iff IoU > thresh; "vote" = bbox_vote, cluster iff IoU >= thresh to the leader, box =
    sum(score * box) / sum(score) in fp32 under the leader's score, source and view the leader's; thresh <= 0: nothing is suppressed.
    Then the cut to top_n over all classes.
    -> (boxes [B, D, 4], scores [B, D], labels, source, view [B, D], count [B]), D = top_n: score descending, then the smaller label, then
    the earlier slot (= the earlier view, then the earlier slot within it); past count the padding of nms_ml and view -1.
    On the device: one int64 sort by (label, score), fiber_det_aug_merge (grid classes x images), one sort by score and gathers; nothing
    is read back.  On CPU tensors the same in numpy."""
    if mode in ("soft-nms", "soft-vote"):
        raise NotImplementedError(f"det_aug_merge: TEST.SPECIAL_NMS {mode!r} is out of scope (soft-nms is a sequential CPU op in the "
                                  "reference; soft-vote appends decayed copies and changes the output size); \"none\" and \"vote\" are built")
    if mode not in DET_AUG_MODES:
        raise ValueError(f"det_aug_merge: mode {mode!r}: \"none\" or \"vote\"")
    if boxes.dim() != 3 or scores.dim() != 2:
        raise ValueError(f"det_aug_merge: boxes {tuple(boxes.shape)}, scores {tuple(scores.shape)}: [B, T, 4] and [B, T]")
    B, T = scores.shape
    if boxes.shape != (B, T, 4) or labels.shape != (B, T) or source.shape != (B, T) or view.shape != (B, T):
        raise ValueError(f"det_aug_merge: boxes {tuple(boxes.shape)}, labels {tuple(labels.shape)}, source {tuple(source.shape)}, view "
                         f"{tuple(view.shape)} for scores {tuple(scores.shape)}")
    if boxes.dtype != torch.float32 or scores.dtype != torch.float32 or labels.dtype != torch.int32 or source.dtype != torch.int32 or \
            view.dtype != torch.int32:
        raise ValueError("det_aug_merge: boxes / scores fp32, labels / source / view int32")
    dev = scores.device
    _det_aug_check_classes(classes, dev, "det_aug_merge")
    if any(t.device != dev for t in (boxes, labels, source, view)):
        raise ValueError("det_aug_merge: the tensors lie on different devices")
    if T > DET_AUG_MAX_CANDIDATES:
        raise ValueError(f"det_aug_merge: {T} candidates per image exceed the capacity of {DET_AUG_MAX_CANDIDATES}")
    D = int(top_n)
    if D <= 0:
        raise ValueError(f"det_aug_merge: top_n {top_n}: the result has the fixed size [B, top_n]")
    thresh, m = float(thresh), DET_AUG_MODES[mode]
    if not scores.is_cuda:
        return _det_aug_merge_host(boxes, scores, labels, source, view, classes, thresh, m, D)
    if B == 0 or T == 0:
        return (torch.zeros((B, D, 4), dtype=torch.float32, device=dev), torch.full((B, D), -1.0, dtype=torch.float32, device=dev),
                torch.zeros((B, D), dtype=torch.int32, device=dev), torch.full((B, D), -1, dtype=torch.int32, device=dev),
                torch.full((B, D), -1, dtype=torch.int32, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev))
    live = scores >= 0
    # one key per slot: label in the high word, the score's bits (monotonic for scores >= 0) inverted in the low one; the stable ascending
    # sort then gives label ascending, score descending, slot ascending, dead slots last
    bits = scores.contiguous().view(torch.int32).clamp_min(0).long()
    key = torch.where(live, (labels.long() << 32) | (0x7FFFFFFF - bits), torch.full_like(bits, _DET_AUG_DEAD << 32))
    key, order = torch.sort(key, dim=1, stable=True)
    s_labels = (key >> 32).to(torch.int32).contiguous()
    s_boxes = torch.gather(boxes, 1, order[:, :, None].expand(-1, -1, 4)).contiguous()
    s_scores = torch.gather(scores, 1, order).contiguous()
    if thresh > 0 and classes.numel() > 0:
        state = torch.zeros((B, T), dtype=torch.int32, device=dev)
        m_boxes = torch.empty((B, T, 4), dtype=torch.float32, device=dev)                # written where state == 1 only
        lib.call("fiber_det_aug_merge", lib.ptr(s_boxes), lib.ptr(s_scores), lib.ptr(s_labels), lib.ptr(_c(classes)), lib.ptr(state),
                 lib.ptr(m_boxes), B, T, int(classes.numel()), thresh, m)
        kept = state == 1
    elif classes.numel() > 0:                                # no suppression: every live candidate of a listed class is kept
        at = torch.searchsorted(classes, s_labels).clamp_(max=classes.numel() - 1)
        kept, m_boxes = torch.gather(live, 1, order) & (classes[at] == s_labels), s_boxes
    else:
        kept, m_boxes = torch.zeros_like(live), s_boxes
    # the cut: the sorted order is (label, score, slot), so a stable sort by score leaves equal scores by label, then slot
    f_scores, pick = torch.sort(torch.where(kept, s_scores, torch.full_like(s_scores, -1.0)), dim=1, descending=True, stable=True)
    f_scores, pick = f_scores[:, :D], pick[:, :D]
    ok = f_scores >= 0
    slot = torch.gather(order, 1, pick)
    o_boxes = torch.where(ok[:, :, None], torch.gather(m_boxes, 1, pick[:, :, None].expand(-1, -1, 4)), torch.zeros((), device=dev))
    o_labels = torch.where(ok, torch.gather(s_labels, 1, pick), torch.zeros((), dtype=torch.int32, device=dev))
    neg = torch.full((), -1, dtype=torch.int32, device=dev)
    o_source = torch.where(ok, torch.gather(source, 1, slot), neg)
    o_view = torch.where(ok, torch.gather(view, 1, slot), neg)
    count = ok.sum(dim=1, dtype=torch.int32)
    if T < D:                                                # fewer slots than the result holds: nms_ml's padding
        pad = D - T
        F = torch.nn.functional
        o_boxes, f_scores = F.pad(o_boxes, (0, 0, 0, pad)), F.pad(f_scores, (0, pad), value=-1.0)
        o_labels, o_source, o_view = F.pad(o_labels, (0, pad)), F.pad(o_source, (0, pad), value=-1), F.pad(o_view, (0, pad), value=-1)
    return o_boxes.contiguous(), f_scores.contiguous(), o_labels.contiguous(), o_source.contiguous(), o_view.contiguous(), count


# ---- grounding evaluation: recall@k of Detections against per-phrase ground truth (csrc/geval.hip) -----------------------------------
def ground_recall(boxes, labels, count, gt, gt_count, cat_mask, topk, positives, totals, thresh, mode, num_categories=64):
    """One launch of fiber_ground_recall, no host synchronisation.  boxes fp32 [B, D, 4] in the original frame, labels int32 [B, D]
    (None in mode 1), count int32 [B], gt fp64 [B, P, G, 4], gt_count int32 [B, P], cat_mask int64 [B, P] (bit 0 = "all"), topk int32
    [K]; positives / totals int64 [K, 64] are accumulated IN PLACE.  mode 0 = Flickr recall, 1 = RefExp precision.
    -> (hit int32 [B, P, K], best fp64 [B, P, K])."""
    B, D = boxes.shape[:2]
    P, G = gt.shape[1:3]
    K = topk.numel()
    if boxes.shape != (B, D, 4) or gt.shape != (B, P, G, 4) or gt_count.shape != (B, P) or cat_mask.shape != (B, P) or count.shape != (B,):
        raise ValueError(f"ground_recall: boxes {tuple(boxes.shape)}, gt {tuple(gt.shape)}, gt_count {tuple(gt_count.shape)}, "
                         f"cat_mask {tuple(cat_mask.shape)}, count {tuple(count.shape)}")
    if gt.dtype != torch.float64 or gt_count.dtype != torch.int32 or cat_mask.dtype != torch.int64 or topk.dtype != torch.int32 or \
            count.dtype != torch.int32 or (labels is not None and (labels.dtype != torch.int32 or labels.shape != (B, D))):
        raise ValueError("ground_recall: gt fp64, gt_count / topk / count / labels int32, cat_mask int64")
    for t in (positives, totals):
        if t.dtype != torch.int64 or t.shape != (K, 64) or not t.is_contiguous():
            raise ValueError("ground_recall: positives / totals are contiguous int64 [K, 64]")
    dev = boxes.device
    hit = torch.empty((B, P, K), dtype=torch.int32, device=dev)
    best = torch.empty((B, P, K), dtype=torch.float64, device=dev)
    lib.call("fiber_ground_recall", lib.ptr(_det_f32(boxes)), lib.ptr(None if labels is None else _c(labels)), lib.ptr(_c(count)),
             lib.ptr(_c(gt)), lib.ptr(_c(gt_count)), lib.ptr(_c(cat_mask)), lib.ptr(_c(topk)), lib.ptr(hit), lib.ptr(best),
             lib.ptr(positives), lib.ptr(totals), B, D, P, G, K, int(num_categories), float(thresh), int(mode))
    return hit, best


# ---- retrieval evaluation: rank of the first matching candidate per query and the recall@k tallies (csrc/retrieval.hip) ---------------
RETRIEVAL_MAX_K = 8


def _retrieval_ranks_host(scores, iids, tiids, ks):
    """fiber_retrieval_ranks on CPU tensors, in torch: a stable descending sort per direction, then the position of the first match"""
    def first_match(s, qid, cid):                            # s [Q, N], qid [Q], cid [N] -> int32 [Q]
        Q, N = s.shape
        if N == 0:
            return torch.zeros(Q, dtype=torch.int32)
        order = torch.sort(s, dim=1, descending=True, stable=True).indices
        same = cid[order] == qid[:, None]
        pos = torch.where(same, torch.arange(N)[None, :], torch.full((), N))
        return pos.min(dim=1).values.to(torch.int32)
    rank_tr = first_match(scores, iids, tiids)
    rank_ir = first_match(scores.t(), tiids, iids)
    hits = torch.stack([(rank_ir[:, None] < ks[None, :]).sum(0), (rank_tr[:, None] < ks[None, :]).sum(0)]).to(torch.int32)
    return rank_tr, rank_ir, hits


def retrieval_ranks(scores, iids, tiids, ks=(1, 5, 10)):
    """Ranks and recall@k tallies of an image-text score matrix (objectives.py:361-383, :477-497 without topk).  scores fp32 [Ni, Nt]
    (row = image, column = text; any row stride, unit column stride), iids int32 [Ni], tiids int32 [Nt]: the image id of each caption;
    ks: up to 8 cut-offs (a sequence or an int32 tensor).  A query's candidates are ordered by descending score, equal scores by
    ascending index; rank = position of the first candidate with the query's id (N when there is none), hit@k = rank < k.
    -> (rank_tr int32 [Ni], rank_ir int32 [Nt], hits int32 [2, nk]: row 0 image retrieval, row 1 text retrieval).  Recall = hits / N (on the
    device form it in fp64 and round once: torch's fp32 division there is not the correctly rounded one).  Two launches, no synchronisation; on CPU tensors the same in torch."""
    if scores.dim() != 2 or scores.dtype != torch.float32:
        raise ValueError(f"retrieval_ranks: scores {tuple(scores.shape)} {scores.dtype}: fp32 [Ni, Nt]")
    Ni, Nt = scores.shape
    dev = scores.device
    if not isinstance(ks, torch.Tensor):
        ks = torch.tensor([int(k) for k in ks], dtype=torch.int32, device=dev)
    if iids.shape != (Ni,) or tiids.shape != (Nt,) or ks.dim() != 1 or iids.dtype != torch.int32 or tiids.dtype != torch.int32 or \
            ks.dtype != torch.int32:
        raise ValueError(f"retrieval_ranks: iids {tuple(iids.shape)} {iids.dtype}, tiids {tuple(tiids.shape)} {tiids.dtype}, ks "
                         f"{tuple(ks.shape)} {ks.dtype} for scores {tuple(scores.shape)}: int32 [Ni], [Nt], [nk]")
    nk = ks.numel()
    if nk > RETRIEVAL_MAX_K:
        raise ValueError(f"retrieval_ranks: {nk} cut-offs exceed the kernel's {RETRIEVAL_MAX_K}")
    if any(t.device != dev for t in (iids, tiids, ks)):
        raise ValueError("retrieval_ranks: the tensors lie on different devices")
    if not scores.is_cuda:
        return _retrieval_ranks_host(scores, iids, tiids, ks)
    if Nt > 1 and scores.stride(1) != 1 or (Ni > 1 and scores.stride(0) < Nt):
        scores = scores.contiguous()
    ld = scores.stride(0) if Ni > 1 else max(Nt, 1)
    rank_tr = torch.empty((Ni,), dtype=torch.int32, device=dev)
    rank_ir = torch.empty((Nt,), dtype=torch.int32, device=dev)
    hits = torch.empty((2, nk), dtype=torch.int32, device=dev)
    lib.call("fiber_retrieval_ranks", lib.ptr(scores), lib.ptr(_c(iids)), lib.ptr(_c(tiids)), lib.ptr(_c(ks)), lib.ptr(rank_tr),
             lib.ptr(rank_ir), lib.ptr(hits), Ni, Nt, int(ld), nk)
    return rank_tr, rank_ir, hits


# ---- box average precision: LVIS-protocol matching and precision / recall tables (csrc/apeval.hip) -----------------------------------
def ap_max_gt():
    return int(lib.plain("fiber_ap_max_gt"))


def ap_chunk():
    return int(lib.plain("fiber_ap_chunk"))


def ap_match(boxes, labels, count, gt, gt_area, gt_cat, gt_ignore, gt_count, neg_mask, nel_mask, iou_thrs, area_rng, num_gt, max_dets):
    """One launch of fiber_ap_match, no host synchronisation.  boxes fp32 [B, D, 4] xyxy in the original frame, labels int32 [B, D]
    (category index + 1), count int32 [B]; gt fp64 [B, G, 4] xywh, gt_area fp64 [B, G], gt_cat int32 [B, G], gt_ignore uint8 [B, G],
    gt_count int32 [B]; neg_mask / nel_mask int64 [B, ceil(C / 64)] (the bits of a uint64); iou_thrs fp64 [T], area_rng fp64 [A, 2];
    num_gt int64 [C, A] is accumulated IN PLACE.  -> (match int64 [B, D], ignore int64 [B, D] (bit a * T + t), valid uint8 [B, D])."""
    B, D = boxes.shape[:2]
    G = gt.shape[1]
    C, A = num_gt.shape
    T = iou_thrs.numel()
    W = (C + 63) // 64
    if boxes.shape != (B, D, 4) or labels.shape != (B, D) or count.shape != (B,) or gt.shape != (B, G, 4) or gt_area.shape != (B, G) or \
            gt_cat.shape != (B, G) or gt_ignore.shape != (B, G) or gt_count.shape != (B,) or neg_mask.shape != (B, W) or \
            nel_mask.shape != (B, W) or area_rng.shape != (A, 2):
        raise ValueError(f"ap_match: boxes {tuple(boxes.shape)}, labels {tuple(labels.shape)}, gt {tuple(gt.shape)}, masks "
                         f"{tuple(neg_mask.shape)} for C = {C}, area_rng {tuple(area_rng.shape)} for A = {A}")
    if labels.dtype != torch.int32 or count.dtype != torch.int32 or gt.dtype != torch.float64 or gt_area.dtype != torch.float64 or \
            gt_cat.dtype != torch.int32 or gt_ignore.dtype != torch.uint8 or gt_count.dtype != torch.int32 or \
            neg_mask.dtype != torch.int64 or nel_mask.dtype != torch.int64 or iou_thrs.dtype != torch.float64 or \
            area_rng.dtype != torch.float64 or num_gt.dtype != torch.int64 or not num_gt.is_contiguous():
        raise ValueError("ap_match: gt / gt_area / iou_thrs / area_rng fp64, labels / count / gt_cat / gt_count int32, gt_ignore uint8, "
                         "masks and num_gt (contiguous) int64")
    if T * A > 64:
        raise ValueError(f"ap_match: {T} thresholds x {A} area ranges exceed the 64 bits of a record's match word")
    if G > ap_max_gt():
        raise ValueError(f"ap_match: {G} ground-truth boxes per image exceed the kernel's capacity of {ap_max_gt()}")
    dev = boxes.device
    match = torch.empty((B, D), dtype=torch.int64, device=dev)
    ignore = torch.empty((B, D), dtype=torch.int64, device=dev)
    valid = torch.empty((B, D), dtype=torch.uint8, device=dev)
    lib.call("fiber_ap_match", lib.ptr(_det_f32(boxes)), lib.ptr(_c(labels)), lib.ptr(_c(count)), lib.ptr(_c(gt)), lib.ptr(_c(gt_area)),
             lib.ptr(_c(gt_cat)), lib.ptr(_c(gt_ignore)), lib.ptr(_c(gt_count)), lib.ptr(_c(neg_mask)), lib.ptr(_c(nel_mask)),
             lib.ptr(_c(iou_thrs)), lib.ptr(_c(area_rng)), lib.ptr(match), lib.ptr(ignore), lib.ptr(valid), lib.ptr(num_gt), B, D, G, C, T, A,
             int(max_dets))
    return match, ignore, valid


def ap_accumulate(match, ignore, seg_ptr, num_gt, rec_thrs, T):
    """One launch of fiber_ap_accumulate.  match / ignore int64 [N]: the kept records ordered by category, then by descending score;
    seg_ptr int64 [C + 1]; num_gt int64 [C, A]; rec_thrs fp64 [R] ascending.  -> (precision fp64 [T, R, C, A], recall fp64 [T, C, A])."""
    C, A = num_gt.shape
    N, R = match.numel(), rec_thrs.numel()
    if match.dtype != torch.int64 or ignore.dtype != torch.int64 or ignore.numel() != N or seg_ptr.dtype != torch.int64 or \
            seg_ptr.shape != (C + 1,) or num_gt.dtype != torch.int64 or rec_thrs.dtype != torch.float64:
        raise ValueError("ap_accumulate: match / ignore int64 [N], seg_ptr int64 [C + 1], num_gt int64 [C, A], rec_thrs fp64 [R]")
    if T * A > 64:
        raise ValueError(f"ap_accumulate: {T} thresholds x {A} area ranges exceed the 64 bits of a record's match word")
    dev = num_gt.device
    precision = torch.empty((T, R, C, A), dtype=torch.float64, device=dev)
    recall = torch.empty((T, C, A), dtype=torch.float64, device=dev)
    lib.call("fiber_ap_accumulate", lib.ptr(_c(match)), lib.ptr(_c(ignore)), lib.ptr(_c(seg_ptr)), lib.ptr(_c(num_gt)), lib.ptr(_c(rec_thrs)),
             lib.ptr(precision), lib.ptr(recall), N, C, T, A, R)
    return precision, recall


def ap_coco_max_categories():
    return int(lib.plain("fiber_ap_coco_max_categories"))


def ap_match_coco(boxes, labels, count, gt, gt_area, gt_cat, gt_crowd, gt_count, iou_thrs, area_rng, num_gt, cap, plus_one=True):
    """One launch of fiber_ap_match_coco (the COCO protocol: crowd rule, cap per (image, category)), no host synchronisation.  boxes fp32
    [B, D, 4] xyxy in the original frame, labels int32 [B, D] (category index + 1), count int32 [B]; gt fp64 [B, G, 4] xywh, gt_area fp64
    [B, G], gt_cat int32 [B, G], gt_crowd uint8 [B, G], gt_count int32 [B]; iou_thrs fp64 [T], area_rng fp64 [A, 2]; num_gt int64 [C, A]
    is accumulated IN PLACE; cap = maxDets[-1]; plus_one: the reference's + TO_REMOVE on the detection's extents.
    -> (match int64 [B, D], ignore int64 [B, D] (bit a * T + t), rank int32 [B, D], valid uint8 [B, D])."""
    B, D = boxes.shape[:2]
    G = gt.shape[1]
    C, A = num_gt.shape
    T = iou_thrs.numel()
    if boxes.shape != (B, D, 4) or labels.shape != (B, D) or count.shape != (B,) or gt.shape != (B, G, 4) or gt_area.shape != (B, G) or \
            gt_cat.shape != (B, G) or gt_crowd.shape != (B, G) or gt_count.shape != (B,) or area_rng.shape != (A, 2):
        raise ValueError(f"ap_match_coco: boxes {tuple(boxes.shape)}, labels {tuple(labels.shape)}, gt {tuple(gt.shape)}, gt_crowd "
                         f"{tuple(gt_crowd.shape)}, area_rng {tuple(area_rng.shape)} for A = {A}")
    if labels.dtype != torch.int32 or count.dtype != torch.int32 or gt.dtype != torch.float64 or gt_area.dtype != torch.float64 or \
            gt_cat.dtype != torch.int32 or gt_crowd.dtype != torch.uint8 or gt_count.dtype != torch.int32 or \
            iou_thrs.dtype != torch.float64 or area_rng.dtype != torch.float64 or num_gt.dtype != torch.int64 or not num_gt.is_contiguous():
        raise ValueError("ap_match_coco: gt / gt_area / iou_thrs / area_rng fp64, labels / count / gt_cat / gt_count int32, gt_crowd uint8, "
                         "num_gt (contiguous) int64")
    if T * A > 64:
        raise ValueError(f"ap_match_coco: {T} thresholds x {A} area ranges exceed the 64 bits of a record's match word")
    if G > ap_max_gt():
        raise ValueError(f"ap_match_coco: {G} ground-truth boxes per image exceed the kernel's capacity of {ap_max_gt()}")
    if C > ap_coco_max_categories():
        raise ValueError(f"ap_match_coco: {C} categories exceed the kernel's {ap_coco_max_categories()} rank counters")
    if int(cap) < 0:
        raise ValueError(f"ap_match_coco: cap {cap}: the largest maxDets, not negative")
    dev = boxes.device
    match = torch.empty((B, D), dtype=torch.int64, device=dev)
    ignore = torch.empty((B, D), dtype=torch.int64, device=dev)
    rank = torch.empty((B, D), dtype=torch.int32, device=dev)
    valid = torch.empty((B, D), dtype=torch.uint8, device=dev)
    lib.call("fiber_ap_match_coco", lib.ptr(_det_f32(boxes)), lib.ptr(_c(labels)), lib.ptr(_c(count)), lib.ptr(_c(gt)), lib.ptr(_c(gt_area)),
             lib.ptr(_c(gt_cat)), lib.ptr(_c(gt_crowd)), lib.ptr(_c(gt_count)), lib.ptr(_c(iou_thrs)), lib.ptr(_c(area_rng)), lib.ptr(match),
             lib.ptr(ignore), lib.ptr(rank), lib.ptr(valid), lib.ptr(num_gt), B, D, G, C, T, A, int(cap), 1 if plus_one else 0)
    return match, ignore, rank, valid


# ---- grounding training: ATSS assignment + GIoU / centerness losses (csrc/atss.hip) --------------------------------------------------
class Assignment:
    """ops.atss_assign's result, fixed shapes: matched int32 [B, A] (-1 unassigned), labels int32 [B, A] (0), reg_targets fp32 [B, A, 4]
    (0), token_targets uint8 [B, A, T] (unassigned: the one-hot on token T - 1), num_pos int32 [B]; anchors fp32 [A, 4] (the levels
    concatenated) and level_off (host list of L + 1 offsets) travel along for the losses."""

    def __init__(self, matched, labels, reg_targets, token_targets, num_pos, anchors, level_off):
        self.matched, self.labels, self.reg_targets, self.token_targets, self.num_pos = matched, labels, reg_targets, token_targets, num_pos
        self.anchors, self.level_off = anchors, level_off


def _level_offsets(anchors_per_level):
    off = [0]
    for a in anchors_per_level:
        if a.dim() != 2 or a.shape[1] != 4:
            raise ValueError(f"atss: anchors of a level are [A_l, 4], got {tuple(a.shape)}")
        off.append(off[-1] + a.shape[0])
    return off


def _host_ints(values):
    import ctypes
    return (ctypes.c_int * len(values))(*values)


def atss_assign(anchors_per_level, targets, topk=9):
    """ATSS target assignment (modeling/rpn/loss.py:626-827) for one anchor per location.  anchors_per_level: the [A_l, 4] tensors of
    AnchorGenerator; targets: boxes fp32 [B, Gmax, 4], labels int32 [B, Gmax], num_gt int32 [B], positive_map uint8 [B, Gmax, 256] on
    the device (modules/grounding_train.py's GroundingTargets).  Tie rules: equal centre distances go to the lowest anchor index, equal
    IoU to the lowest gt index.  -> Assignment; no host synchronisation, no data-dependent shape."""
    off = _level_offsets(anchors_per_level)
    L, A = len(anchors_per_level), off[-1]
    hoff = _host_ints(off)
    K = lib.plain("fiber_atss_num_candidates", hoff, L, int(topk))
    if K < 0:
        raise lib.FiberHipError(f"atss_assign: {L} levels of sizes {[b - a for a, b in zip(off, off[1:])]} with topk {topk}: the candidates "
                                "per gt must number 2..128 (below 2 the reference's std is NaN) on at most 8 levels")
    boxes, labels = _det_f32(targets.boxes), _c(targets.labels.to(torch.int32))
    num_gt, pmap = _c(targets.num_gt.to(torch.int32)), _c(targets.positive_map.to(torch.uint8))
    B, G = boxes.shape[:2]
    T = pmap.shape[-1]
    if boxes.shape != (B, G, 4) or labels.shape != (B, G) or num_gt.shape != (B,) or pmap.shape != (B, G, T):
        raise ValueError(f"atss_assign: boxes {tuple(boxes.shape)}, labels {tuple(labels.shape)}, num_gt {tuple(num_gt.shape)}, "
                         f"positive_map {tuple(pmap.shape)}")
    dev = boxes.device
    anchors = _c(torch.cat([a.detach().float() for a in anchors_per_level], dim=0))
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)      # noqa: E731  (every element is written by the kernels)
    cand_idx, cand_iou, key = e((B, G, K), torch.int32), e((B, G, K), torch.float32), e((B, A), torch.int64)
    out = Assignment(e((B, A), torch.int32), e((B, A), torch.int32), e((B, A, 4), torch.float32), e((B, A, T), torch.uint8),
                     e((B,), torch.int32), anchors, off)
    lib.call("fiber_atss_candidates_f32", lib.ptr(anchors), hoff, L, lib.ptr(boxes), lib.ptr(num_gt), lib.ptr(cand_idx), lib.ptr(cand_iou),
             B, G, A, int(topk))
    lib.call("fiber_atss_resolve_f32", lib.ptr(anchors), lib.ptr(boxes), lib.ptr(num_gt), lib.ptr(cand_idx), lib.ptr(cand_iou), lib.ptr(key),
             B, G, A, K)
    lib.call("fiber_atss_finalize_f32", lib.ptr(anchors), lib.ptr(boxes), lib.ptr(labels), lib.ptr(pmap), lib.ptr(key), lib.ptr(out.matched),
             lib.ptr(out.labels), lib.ptr(out.reg_targets), lib.ptr(out.token_targets), lib.ptr(out.num_pos), B, G, A, T)
    return out


class _AtssBoxLosses(torch.autograd.Function):
    """Forward: one launch per level into per-workgroup partials + one fold; backward: one launch per level writing the NCHW gradients.
    Returns fp32 [3] = (sum w (1 - giou), sum w, sum BCE(centerness, w)); its upstream gradient is read from device memory."""

    @staticmethod
    def forward(ctx, anchors, labels, reg_targets, level_off, *levels):
        L = len(level_off) - 1
        regs, ctrs = [_det_f32(t) for t in levels[:L]], [_det_f32(t) for t in levels[L:]]
        B, A = labels.shape
        rows = [lib.plain("fiber_atss_loss_rows", B, level_off[l + 1] - level_off[l]) for l in range(L)]
        part = torch.empty((max(1, sum(rows)), 3), dtype=torch.float32, device=labels.device)
        sums = torch.zeros(3, dtype=torch.float32, device=labels.device)
        row0 = 0
        for l in range(L):
            lib.call("fiber_atss_loss_fwd_f32", lib.ptr(regs[l]), lib.ptr(ctrs[l]), lib.ptr(anchors), lib.ptr(labels), lib.ptr(reg_targets),
                     lib.ptr(part), None, B, A, level_off[l + 1] - level_off[l], level_off[l], row0)
            row0 += rows[l]
        if row0:
            lib.call("fiber_fold_rows_f32", lib.ptr(part), lib.ptr(sums), row0, 3)
        ctx.save_for_backward(anchors, labels, reg_targets, *regs, *ctrs)
        ctx.level_off = level_off
        ctx.meta = [(t.shape, t.dtype) for t in levels]
        return sums

    @staticmethod
    def backward(ctx, g):
        anchors, labels, reg_targets, *saved = ctx.saved_tensors
        off = ctx.level_off
        L = len(off) - 1
        B, A = labels.shape
        g32 = _c(g.detach().float().reshape(3))
        dregs, dctrs = [], []
        for l in range(L):
            reg, ctr = saved[l], saved[L + l]
            dreg, dctr = torch.empty_like(reg), torch.empty_like(ctr)
            lib.call("fiber_atss_loss_bwd_f32", lib.ptr(reg), lib.ptr(ctr), lib.ptr(anchors), lib.ptr(labels), lib.ptr(reg_targets),
                     lib.ptr(g32), lib.ptr(dreg), lib.ptr(dctr), B, A, off[l + 1] - off[l], off[l])
            dregs.append(dreg), dctrs.append(dctr)
        grads = [d.view(s).to(dt) for d, (s, dt) in zip(dregs + dctrs, ctx.meta)]
        return (None, None, None, None, *grads)


def atss_box_losses(bbox_reg_levels, centerness_levels, anchors_per_level, assignment):
    """The box-regression and centerness loss sums over the assigned anchors (loss.py:583-624, :829-844, :1237-1254) with bbox_reg
    [B, 4, H, W] and centerness [B, 1, H, W] read in place per level.  -> (sum w (1 - giou), sum w, sum BCE(centerness, w)), w the
    centerness target; differentiable in bbox_reg and centerness; all three are 0 when nothing is assigned."""
    off = _level_offsets(anchors_per_level)
    if off != list(assignment.level_off):
        raise ValueError(f"atss_box_losses: level offsets {off} differ from the assignment's {assignment.level_off}")
    L, (B, A) = len(off) - 1, assignment.labels.shape
    if len(bbox_reg_levels) != L or len(centerness_levels) != L:
        raise ValueError(f"atss_box_losses: {len(bbox_reg_levels)} / {len(centerness_levels)} prediction levels for {L} anchor levels")
    for l, (r, c) in enumerate(zip(bbox_reg_levels, centerness_levels)):
        n = off[l + 1] - off[l]
        if r.shape[0] != B or r.numel() != B * 4 * n or c.numel() != B * n:
            raise NotImplementedError(f"atss_box_losses level {l}: bbox_reg {tuple(r.shape)} / centerness {tuple(c.shape)} for {n} anchors "
                                      "(one anchor per location)")
    sums = _AtssBoxLosses.apply(assignment.anchors, assignment.labels, assignment.reg_targets, off, *bbox_reg_levels, *centerness_levels)
    return sums[0], sums[1], sums[2]


# ---- FPN neck: DropBlock mask + lateral / nearest-upsample merge (csrc/fpn.hip) ----------------------------------------------------
def dropblock_mask(B, H, W, drop_prob, block, device, seeds=None):
    """layers/dropblock.py:42-51, :61-77 -> (keep uint8 [B, H, W], kept int32 [1] = keep.sum(), both on the device; nothing is read on the
    host).  seeds None: the Bernoulli(drop_prob / block^2) draw comes from the dropout key stream (next_seed: capturable in a hipGraph);
    seeds given ([B, H, W], non-zero = block centre): they are used as they are -- how a test replays the reference's own draws."""
    gamma = float(drop_prob) / float(block * block)
    keep = torch.empty((B, H, W), dtype=torch.uint8, device=device)
    kept = torch.empty(1, dtype=torch.int32, device=device)
    if seeds is None:
        s8, draw, seed, base = torch.empty((B, H, W), dtype=torch.uint8, device=device), 1, next_seed(), seed_base_ptr()
    else:
        if tuple(seeds.shape) != (B, H, W):
            raise ValueError(f"dropblock_mask: seeds {tuple(seeds.shape)} for a [{B}, {H}, {W}] map")
        s8, draw, seed, base = (seeds != 0).to(device=device, dtype=torch.uint8).contiguous(), 0, 0, None
    lib.call("fiber_dropblock_mask_u8", lib.ptr(s8), draw, seed, base, gamma, int(block), lib.ptr(keep), lib.ptr(kept), B, H, W)
    return keep, kept


class _FpnMerge(torch.autograd.Function):
    """(inner, dropped) = (lateral + nearest_up(coarse), that * keep * numel / kept) in one launch; backward: one launch for both
    gradients.  coarse / keep may be None; either output's gradient may be None."""

    @staticmethod
    def forward(ctx, lateral, coarse, keep, kept):
        lateral = _c(lateral)
        coarse = _c(coarse) if coarse is not None else None
        B, H, W, C = lateral.shape
        Hc, Wc = (coarse.shape[1], coarse.shape[2]) if coarse is not None else (H, W)
        inner = torch.empty_like(lateral)
        dropped = torch.empty_like(lateral) if keep is not None else None
        lib.call("fiber_fpn_merge_fwd_bf16", lib.ptr(lateral), lib.ptr(coarse), lib.ptr(keep), lib.ptr(kept), lib.ptr(inner), lib.ptr(dropped),
                 B, H, W, C, Hc, Wc)
        ctx.save_for_backward(keep, kept)
        ctx.geom = (B, H, W, C, Hc, Wc, coarse is not None)
        ctx.set_materialize_grads(False)
        if dropped is None:
            return inner, None
        return inner, dropped

    @staticmethod
    def backward(ctx, d_inner, d_dropped):
        keep, kept = ctx.saved_tensors
        B, H, W, C, Hc, Wc, has_coarse = ctx.geom
        ref = d_inner if d_inner is not None else d_dropped
        if ref is None:
            return None, None, None, None
        d_inner = _c(d_inner.to(BF16)) if d_inner is not None else None
        d_dropped = _c(d_dropped.to(BF16)) if d_dropped is not None else None
        d_lat = torch.empty((B, H, W, C), dtype=BF16, device=ref.device)
        d_coarse = torch.empty((B, Hc, Wc, C), dtype=BF16, device=ref.device) if has_coarse else None
        lib.call("fiber_fpn_merge_bwd_bf16", lib.ptr(d_inner), lib.ptr(d_dropped), lib.ptr(keep), lib.ptr(kept), lib.ptr(d_lat),
                 lib.ptr(d_coarse), B, H, W, C, Hc, Wc)
        return d_lat, d_coarse, None, None


def fpn_merge(lateral, coarse, keep=None, kept=None):
    """FPN top-down step on channels-last bf16 maps (fpn.py:97-110): inner = lateral [B, H, W, C] + coarse [B, Hc, Wc, C] up-sampled to
    H x W by F.interpolate's nearest rule; with (keep, kept) of dropblock_mask also dropped = inner * keep * (B H W / kept) formed from the
    unrounded sum.  -> (inner, dropped or None).  coarse None: inner = lateral (DropBlock on a map of its own)."""
    if lateral.dtype != BF16 or lateral.dim() != 4 or (coarse is not None and (coarse.dtype != BF16 or coarse.dim() != 4
                                                                              or coarse.shape[0] != lateral.shape[0] or coarse.shape[3] != lateral.shape[3])):
        raise ValueError(f"fpn_merge: lateral {tuple(lateral.shape)} {lateral.dtype}, coarse {None if coarse is None else tuple(coarse.shape)}")
    if (keep is None) != (kept is None):
        raise ValueError("fpn_merge: keep and kept come together (ops.dropblock_mask)")
    if keep is not None:
        if tuple(keep.shape) != tuple(lateral.shape[:3]) or keep.dtype != torch.uint8 or kept.dtype != torch.int32:
            raise ValueError(f"fpn_merge: keep {tuple(keep.shape)} {keep.dtype} for lateral {tuple(lateral.shape)}")
        keep = keep.contiguous()
    return _FpnMerge.apply(lateral, coarse, keep, kept)


def _weight_2d(weight):
    """The [N, K] view of a [N, K, 1, 1] convolution parameter, ONE object per parameter: the bf16 working copies are keyed by tensor
    identity, so a fresh .view per call would rebuild them every time.  It shares the parameter's storage and version counter."""
    key = ("V2", id(weight))
    hit = _cache_get(key, weight)
    if hit is not None and hit[1].data_ptr() == weight.data_ptr():
        return hit[1]
    v = weight.detach().view(weight.shape[0], weight.shape[1])
    _cache_put(key, None, v, weight)
    return v


class _Conv1x1(torch.autograd.Function):
    """1x1 convolution on channels-last tokens [..., Cin] with an nn.Conv2d-shaped weight: the NT GEMM on the tokens as they lie (no
    im2col copy), dX on the NT kernel, dW / db on the TN kernel."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        shp = x.shape
        x2 = _c(x).view(-1, shp[-1])
        w2 = _weight_2d(weight)
        y, _ = gemm_nt(x2, bf16_weight(w2), bias)
        ctx.save_for_backward(x2, weight)
        ctx.shp, ctx.has_bias = shp, bias is not None
        return y.view(*shp[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, weight = ctx.saved_tensors
        dy2 = _c(dy.to(BF16)).view(-1, weight.shape[0])
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _dgrad(dy2, _weight_2d(weight)).view(ctx.shp)
        need_db = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            dw = wgrad(dy2, x2, want_bias=need_db)
            if need_db:
                dw, db = dw
            dw = dw.view(weight.shape)
        elif need_db:
            db = colsum(dy2)
        return dx, dw, db


def conv1x1(x, weight, bias=None):
    """nn.Conv2d(Cin, Cout, 1) on channels-last bf16 tokens [..., Cin] -> [..., Cout] (the FPN laterals, fpn.py:48, :95)."""
    if weight.dim() != 4 or weight.shape[2:] != (1, 1) or (weight.shape[0] % 8) or (weight.shape[1] % 8):
        raise lib.FiberHipError(f"conv1x1: weight {tuple(weight.shape)} (1x1, channel counts multiples of 8)")
    return _Conv1x1.apply(x, weight, bias)
