"""Case table of the attention path matrix: every kernel template that the four public entry points (fiber_window_attn_*,
fiber_mha_*, fiber_mha_causal_*) reach with the default environment, at a shape that sends the call to it, with the kernels
the forward and the backward must launch.  Shared by tests/test_hip_attn_paths.py (values against fp64, written region) and
tools/probes/attn_paths.py (which kernels each case actually launched).  Also: the fp64 reference and its per-element bounds,
used on the GPU by the path tests and on the host by tests/test_attn_compare_host.py.

Selection, as read from the dispatch (win_attn.hip win_plan(), one per pass, whose form launch_form() maps to a template; attn_x.hip
fiber_*_launch, which alone decide whether a one-pass kernel serves a call -- attn.hip's mha_fwd / mha_bwd add only the head_dim and,
for i2t, "no dropout"; attn.hip attn_plan() and launch_fwd / launch_dq / launch_dkv for the generic kernels):
  window, N = ws*ws <= 160, N != 144   win_fwd_kernel<1, 0>, win_bwd_dq / dkv_kernel<1, 0>; dbias fold (fold1 when heads*N*N % 4 != 0)
  window, N == 144                      win_fwd_kernel<1, 9>, win_bwd_fused_kernel<shift > 0>
  window, 160 < N <= 336                win_fwd_kernel<3, 0, 21, false>, win_bwd_dq / dkv_kernel<3, 0, 21, false>
  (every window form: runs of ceil(G / min(G, (256, from 8 heads * strip groups on 512) / (heads * strip groups))) windows per workgroup)
  window, N > 336                       attn_fwd_kernel<32, true>, attn_delta_kernel, attn_bwd_dq / dkv_kernel<32, true>, dbias_scatter
  mha, D = 32, Lk <= 48, no dropout     i2t_fwd_kernel if Lq % 16 == 0 and heads % 4 == 0; i2t_bwd_kernel if also lddq % 8 == 0
  mha, D = 64, Lq <= 48, Lk <= 1024     t2i_fwd_kernel<DROP>, t2i_bwd_kernel<DROP> (all leading dimensions % 8 == 0)
  mha otherwise                         one attn_plan() per pass: the staged side (forward, dQ: keys; dK/dV: queries) is cut into equal
                                        chunks of at most 10 tiles of 16 rows (8 forward / 5 backward for workgroups of <= 4 waves), and the
                                        chunk's tiles pick the slot form: attn_fwd_kernel<D, false, 4 | 10> (<= 4 tiles or more),
                                        attn_bwd_dq_kernel<D, false, 4 | 6 | 10> (<= 4, <= 6, more), attn_bwd_dkv_kernel<D, false, 4 | 10>
  causal, D = 64, L <= 48               t2i_*_kernel<DROP, true>;  otherwise attn_*_kernel<D, false, 4, true> (L <= 64: one chunk of <= 4 tiles)
A (mode, slots) pair outside this list is refused by the launchers (FIBER_EINVAL), not served by another template; the window mode of the
generic kernels exists for head_dim 32 only.
Not reached by default: win_bwd_fused_kernel<*, 11> (FIBER_WIN_BWD_WAVES=11).
A sample whose every key is masked with finfo(fp32).min ("allmin") is the uniform average, as the reference's fp32 softmax gives it
(finfo.min absorbs the scores); the kernels replace such scores by KMASK_SCORE (common.h), so its lse is private to the kernels."""
import math

import torch

U = 2.0 ** -8                 # bf16 store: |bf16(v) - v| <= 2^-8 |v|
TINY = 2.0 ** -100            # absolute: sums of terms of probabilities below fp32's normal range, which the kernels flush to zero
# bound constants (tests/test_hip_attn_paths.py), each named after the rounding it covers; set on the first MI355X run as the smallest
# power of two that passes every case, not to be raised to admit a change
# (first MI355X run, each constant with the others at 2^-20 / 2^-8 / 2^-8: the largest value any element needed)
CONST = {
    "C_S": 2.0 ** -25,        # fp32 score, log2e fold, exp2 and lse, in units of P * E (E = A + |s|); needed 2^-25.76, causal32-L40-pad lse
    "C_PV": 2.0 ** -8,        # P (times the dropout factor) rounded to bf16 for the PV / P^T dO MFMAs + fp32 accumulation; needed 2^-8.22,
                              # causal64-L17-min dv
    "C_DS": 2.0 ** -9,        # dS rounded to bf16 for the dQ / dK MFMAs; delta from the stored bf16 O; needed 2^-9.76, w12s-spike-last dq
    "C_SUM": 2.0 ** -16,      # fp32 sums over windows (dbias_table) and rows (column sums), in units of the sums of magnitudes; no
                              # case needed it beyond the per-entry dS terms (kept at the GEMM column sums' value)
}
NAN_BF16 = 0x7FA5             # fill pattern of output buffers (a quiet NaN no kernel computes)
NAN_F32 = 0x7FC0ABCD
FINFO_MIN = torch.finfo(torch.float32).min
KMASK_SCORE_NAT = 16000.0 * math.log(2.0)     # |the score a finfo.min-masked key gets in the kernels| (common.h KMASK_SCORE), natural log

_WF = "win_fwd_kernel<1, 0, 10, true>"
_WF12 = "win_fwd_kernel<1, 9, 10, true>"
_WF21 = "win_fwd_kernel<3, 0, 21, false>"


def _fold(heads, N):
    return "win_dbias_fold_kernel" if heads * N * N % 4 == 0 else "win_dbias_fold1_kernel"


def window_kernels(c):
    """(forward, backward) kernel templates of a window case, as the profiler spells them (with the column-sum fold)."""
    N, h = c["ws"] ** 2, c["heads"]
    if N > 336:
        return [f"attn_fwd_kernel<32, true, 10, false>"], ["attn_delta_kernel<32>", "attn_bwd_dq_kernel<32, true, 10, false>",
                                                          "dbias_scatter_kernel", "attn_bwd_dkv_kernel<32, true, 10, false>"]
    tail = [_fold(h, N), "win_dbias_gather_kernel"] + (["colsum_fold_kernel"] if c["colsum"] else [])
    if N > 160:
        return [_WF21], ["win_bwd_dq_kernel<3, 0, 21, false>", "win_bwd_dkv_kernel<3, 0, 21, false>"] + tail
    if N == 144:
        return [_WF12], [f"win_bwd_fused_kernel<{'true' if c['shift'] else 'false'}, 9>"] + tail
    return [_WF], ["win_bwd_dq_kernel<1, 0, 10, true>", "win_bwd_dkv_kernel<1, 0, 10, true>"] + tail


def _win(name, B, H, W, heads, ws, shift, layout=0, colsum=False, inputs="rand"):
    c = dict(kind="window", name=name, B=B, H=H, W=W, heads=heads, ws=ws, shift=shift, layout=layout, colsum=colsum, inputs=inputs)
    c["fwd"], c["bwd"] = window_kernels(c)
    return c


WIN_CASES = []
# (name, B, H, W, heads, ws, shift, layouts): every window template with and without the shift, in every layout the ABI accepts
for nm, B, H, W, h, ws, s, lays in [
    ("w3", 2, 6, 6, 1, 3, 0, (0, 1, 2)), ("w3s", 2, 6, 6, 3, 3, 1, (0, 1, 2)),        # one partial strip; H*N*N odd -> fold1
    ("w7", 2, 14, 14, 3, 7, 0, (0,)), ("w7s", 2, 14, 14, 2, 7, 3, (0, 2)),
    ("w8", 2, 16, 16, 2, 8, 0, (0, 1)), ("w8s", 1, 16, 16, 4, 8, 4, (0, 1, 2)),
    ("w12", 2, 24, 24, 4, 12, 0, (0, 1, 2)), ("w12s", 1, 24, 24, 4, 12, 6, (0, 1, 2)),
    ("w13", 1, 26, 26, 2, 13, 0, (0, 1, 2)), ("w13s", 1, 26, 26, 2, 13, 6, (0, 2)),
    ("w18", 2, 18, 18, 4, 18, 0, (0, 1)), ("w18s", 1, 36, 36, 2, 18, 9, (0, 1, 2)),
    ("w19", 1, 38, 38, 2, 19, 0, (0,)), ("w19s", 1, 38, 38, 2, 19, 9, (0,)),          # generic: 361 rows = three 160-row chunks
    ("w24", 1, 48, 24, 2, 24, 0, (0,)), ("w24s", 1, 48, 24, 2, 24, 12, (0,)),          # generic, rectangular
    # rectangular padded grid; shifted single-window grids; ragged last window run (G not a multiple of gpb)
    ("w12rect", 1, 24, 36, 4, 12, 6, (0,)), ("w12one", 2, 12, 12, 2, 12, 6, (0,)), ("w7one", 2, 7, 7, 2, 7, 3, (0,)),
    ("w12rag", 33, 24, 24, 16, 12, 6, (0,)), ("w7rag", 35, 14, 14, 4, 7, 3, (0,)), ("w18rag", 33, 18, 18, 16, 18, 0, (0,)),
    ("w7rag8", 1, 63, 63, 8, 7, 3, (0,)),      # the two-pass kernels at >= 8 heads: 81 windows in 41 runs of two, the last run one window
    ("w18bench", 8, 18, 18, 32, 18, 0, (0,)),                                         # the bench's stage 3 at 576^2 (Swin-B, 32 heads)
]:
    for lay in lays:
        WIN_CASES.append(_win(f"{nm}-l{lay}", B, H, W, h, ws, s, lay, colsum=ws * ws <= 336))
# numerical edges: scores over +-60 with each row's maximum in the last / first key chunk; shift-masked keys that dominate
WIN_CASES += [
    _win("w19-spike-last", 1, 38, 38, 2, 19, 9, inputs="spike_last"), _win("w19-spike-first", 1, 38, 38, 2, 19, 9, inputs="spike_first"),
    _win("w12s-spike-last", 1, 24, 24, 4, 12, 6, colsum=True, inputs="spike_last"),
    _win("w18s-spike-first", 1, 36, 36, 2, 18, 9, colsum=True, inputs="spike_first"),
    _win("w7s-shiftdom", 1, 14, 14, 2, 7, 3, colsum=True, inputs="shift_dominant"),
    _win("w12s-shiftdom", 1, 24, 24, 2, 12, 6, colsum=True, inputs="shift_dominant"),
    _win("w18s-shiftdom", 1, 36, 36, 2, 18, 9, colsum=True, inputs="shift_dominant"),
    _win("w19s-shiftdom", 1, 38, 38, 2, 19, 9, inputs="shift_dominant"),
]

_GF = lambda D, nt, causal=False: f"attn_fwd_kernel<{D}, false, {nt}, {'true' if causal else 'false'}>"
_GQ = lambda D, nt, causal=False: f"attn_bwd_dq_kernel<{D}, false, {nt}, {'true' if causal else 'false'}>"
_GK = lambda D, nt, causal=False: f"attn_bwd_dkv_kernel<{D}, false, {nt}, {'true' if causal else 'false'}>"
_GB = lambda D, nq, nk, causal=False: [f"attn_delta_kernel<{D}>", _GQ(D, nq, causal), _GK(D, nk, causal)]
_TF = lambda drop, causal=False: f"t2i_fwd_kernel<{'true' if drop else 'false'}, {'true' if causal else 'false'}>"
_TB = lambda drop, causal=False: f"t2i_bwd_kernel<{'true' if drop else 'false'}, {'true' if causal else 'false'}>"


def _mha(name, B, heads, Lq, Lk, D, fwd, bwd, mask="pad", p=0.0, causal=False, packed=False, pad=8, lddq=None, lddk=None,
         inputs="rand"):
    """pad: extra columns of every leading dimension; lddq / lddk: overrides (mixed paths); packed: self-attention whose gradient is
    one [B*L, 3C] buffer (as _MHAPacked writes it)."""
    C = heads * D
    c = dict(kind="mha", name=name, B=B, heads=heads, Lq=Lq, Lk=Lk, D=D, mask=mask, p=p, causal=causal, packed=packed, inputs=inputs,
             fwd=list(fwd), bwd=list(bwd))
    c["ld"] = dict(q=C + pad, k=C + 2 * pad, v=C + pad, o=C + pad, do=C + 2 * pad, dq=lddq or C + pad, dk=lddk or C + pad, dv=C + 2 * pad)
    if packed:
        assert Lq == Lk
        c["ld"].update(dq=3 * C + pad, dk=3 * C + pad, dv=3 * C + pad)
    return c


MHA_CASES = [
    # image -> text: the one-pass i2t kernels (D = 32, <= 48 keys, Lq % 16 == 0, heads % 4 == 0) and their edges
    _mha("i2t", 2, 8, 64, 40, 32, ["i2t_fwd_kernel"], ["i2t_bwd_kernel"]),
    _mha("i2t-lk48", 2, 4, 48, 48, 32, ["i2t_fwd_kernel"], ["i2t_bwd_kernel"], mask="none", packed=True),
    _mha("i2t-lk1", 2, 4, 16, 1, 32, ["i2t_fwd_kernel"], ["i2t_bwd_kernel"], mask="none"),
    _mha("i2t-allpad", 3, 4, 32, 17, 32, ["i2t_fwd_kernel"], ["i2t_bwd_kernel"], mask="allpad"),
    _mha("i2t-allmin", 3, 4, 32, 17, 32, ["i2t_fwd_kernel"], ["i2t_bwd_kernel"], mask="allmin"),
    # mixed: i2t forward, generic backward (lddq % 8 == 4)
    _mha("i2t-mixed", 2, 8, 64, 40, 32, ["i2t_fwd_kernel"], _GB(32, 4, 4), lddq=8 * 32 + 4),
    _mha("i2t-mixed-allmin", 2, 4, 32, 40, 32, ["i2t_fwd_kernel"], _GB(32, 4, 4), mask="allmin", lddq=4 * 32 + 4),
    # just outside i2t: 6 heads, a ragged query strip, 49 keys, dropout
    _mha("g32-h6", 2, 6, 64, 40, 32, [_GF(32, 4)], _GB(32, 4, 4)),
    _mha("g32-ragq", 2, 4, 72, 40, 32, [_GF(32, 4)], _GB(32, 4, 10)),
    _mha("g32-lk49", 2, 4, 64, 49, 32, [_GF(32, 4)], _GB(32, 4, 4)),
    _mha("g32-drop", 2, 4, 64, 40, 32, [_GF(32, 4)], _GB(32, 4, 4), p=0.1),
    # generic head_dim 32: multi-chunk forward (Lk > 160), 6- and 10-slot dQ, 10-slot dK/dV, ragged strips, one key
    _mha("g32-lk200", 2, 3, 64, 200, 32, [_GF(32, 10)], _GB(32, 6, 4)),
    _mha("g32-200x200", 2, 2, 200, 200, 32, [_GF(32, 10)], _GB(32, 10, 10), packed=True),
    _mha("g32-9x70", 3, 5, 9, 70, 32, [_GF(32, 10)], _GB(32, 6, 4)),
    _mha("g32-lk1", 2, 3, 50, 1, 32, [_GF(32, 4)], _GB(32, 4, 4)),
    _mha("g32-lk200-drop", 2, 3, 64, 200, 32, [_GF(32, 10)], _GB(32, 6, 4), p=0.1),
    _mha("g32-lk200-spike-last", 2, 2, 64, 200, 32, [_GF(32, 10)], _GB(32, 6, 4), mask="none", inputs="spike_last"),
    _mha("g32-lk200-spike-first", 2, 2, 64, 200, 32, [_GF(32, 10)], _GB(32, 6, 4), mask="none", inputs="spike_first"),
    _mha("g32-allpad", 3, 3, 64, 100, 32, [_GF(32, 10)], _GB(32, 4, 4), mask="allpad"),
    _mha("g32-allmin", 3, 3, 64, 100, 32, [_GF(32, 10)], _GB(32, 4, 4), mask="allmin"),
    # text -> image / text self-attention: the one-pass t2i kernels (D = 64, <= 48 queries, <= 1024 keys), with and without dropout
    _mha("t2i", 2, 3, 40, 576, 64, [_TF(False)], [_TB(False)]),
    _mha("t2i-drop", 2, 3, 40, 576, 64, [_TF(True)], [_TB(True)], p=0.1),
    _mha("t2i-self", 2, 5, 40, 40, 64, [_TF(False)], [_TB(False)], packed=True),
    _mha("t2i-self-drop", 2, 5, 33, 33, 64, [_TF(True)], [_TB(True)], p=0.1, packed=True),
    _mha("t2i-lk1024", 1, 2, 48, 1024, 64, [_TF(False)], [_TB(False)]),
    _mha("t2i-lq1-lk1", 2, 3, 1, 1, 64, [_TF(False)], [_TB(False)], mask="none"),
    _mha("t2i-spike-last", 2, 2, 40, 576, 64, [_TF(False)], [_TB(False)], mask="none", inputs="spike_last"),
    _mha("t2i-spike-first", 2, 2, 40, 576, 64, [_TF(False)], [_TB(False)], mask="none", inputs="spike_first"),
    _mha("t2i-allpad", 3, 2, 40, 100, 64, [_TF(False)], [_TB(False)], mask="allpad"),
    _mha("t2i-allmin", 3, 2, 40, 100, 64, [_TF(False)], [_TB(False)], mask="allmin"),
    # 1025 keys: past T_MAXK, both directions fall back to the generic kernels
    _mha("t2i-lk1025", 1, 2, 40, 1025, 64, [_GF(64, 10)], _GB(64, 6, 4)),
    # mixed: t2i forward, generic backward (lddk % 8 == 4)
    _mha("t2i-mixed", 2, 3, 40, 144, 64, [_TF(False)], _GB(64, 6, 4), lddk=3 * 64 + 4),
    _mha("t2i-mixed-allmin", 3, 2, 40, 100, 64, [_TF(False)], _GB(64, 4, 4), mask="allmin", lddk=2 * 64 + 4),
    # generic head_dim 64 (> 48 queries)
    _mha("g64-4", 2, 5, 64, 50, 64, [_GF(64, 4)], _GB(64, 4, 4)),
    _mha("g64-lk200", 2, 3, 64, 200, 64, [_GF(64, 10)], _GB(64, 6, 4)),
    _mha("g64-200x200", 2, 2, 200, 200, 64, [_GF(64, 10)], _GB(64, 10, 10)),
    _mha("g64-200x200-drop", 1, 2, 200, 200, 64, [_GF(64, 10)], _GB(64, 10, 10), p=0.1, packed=True),
    _mha("g64-lk1", 2, 3, 60, 1, 64, [_GF(64, 4)], _GB(64, 4, 4)),
    _mha("g64-allmin", 2, 3, 64, 50, 64, [_GF(64, 4)], _GB(64, 4, 4), mask="allmin"),
    # launch geometry (attn_plan; profiles/attn_dispatch.md lists the branches): a capped grid whose 3-wave workgroups loop over query
    # strips (forward, dQ: heads * B * 12 > 2048) or whose 8-wave workgroups loop over key strips (dK/dV: heads * B * 3 > 2048); 9 waves cut
    # to the 8 that the 10-slot dQ form (18 strips) and the 10-slot D = 64 dQ and dK/dV forms (9 strips) are built for
    _mha("g32-gridcap", 32, 6, 576, 40, 32, [_GF(32, 4)], _GB(32, 4, 10)),
    _mha("g32-dkv-gridcap", 64, 16, 16, 257, 32, [_GF(32, 10)], _GB(32, 6, 4)),
    _mha("g32-288x200", 2, 2, 288, 200, 32, [_GF(32, 10)], _GB(32, 10, 10)),
    _mha("g64-144x144", 2, 2, 144, 144, 64, [_GF(64, 10)], _GB(64, 10, 10)),
]

CAUSAL_CASES = []
for D, L in [(64, 40), (64, 48), (64, 1), (64, 17), (32, 1), (32, 40), (32, 64), (64, 49), (64, 64)]:
    one = D == 64 and L <= 48
    fwd = [_TF(False, True)] if one else [_GF(D, 4, True)]
    bwd = [_TB(False, True)] if one else _GB(D, 4, 4, True)
    for mask in (("none",) if L == 1 else ("none", "pad", "min")):
        CAUSAL_CASES.append(_mha(f"causal{D}-L{L}-{mask}", 2, 3, L, L, D, fwd, bwd, mask=mask, causal=True, packed=mask == "pad"))
    if L in (40, 64):
        drop_fwd = [_TF(True, True)] if one else fwd
        drop_bwd = [_TB(True, True)] if one else bwd
        CAUSAL_CASES.append(_mha(f"causal{D}-L{L}-drop", 2, 3, L, L, D, drop_fwd, drop_bwd, mask="pad", p=0.1, causal=True))
CAUSAL_CASES += [
    _mha("causal64-L40-allmin", 3, 2, 40, 40, 64, [_TF(False, True)], [_TB(False, True)], mask="allmin", causal=True),
    _mha("causal32-L40-allmin", 3, 2, 40, 40, 32, [_GF(32, 4, True)], _GB(32, 4, 4, True), mask="allmin", causal=True),
    _mha("causal64-L64-allmin", 3, 2, 64, 64, 64, [_GF(64, 4, True)], _GB(64, 4, 4, True), mask="allmin", causal=True),
    _mha("causal64-L40-allpad", 3, 2, 40, 40, 64, [_TF(False, True)], [_TB(False, True)], mask="allpad", causal=True),
]

CASES = WIN_CASES + MHA_CASES + CAUSAL_CASES
CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------------------------------ window geometry
def window_geometry(B, H, W, ws, shift, device="cpu"):
    """tok [G, N]: the image-token row of window g's local token i (roll by -shift, partition); reg [G, N] the Swin shift-region label
    of that token inside its window (all 0 without a shift); rel [N, N] the bias-table index of (i, j)."""
    nWh, nWw = H // ws, W // ws
    wr = torch.arange(nWh, device=device)[:, None, None, None]
    wc = torch.arange(nWw, device=device)[None, :, None, None]
    lr = torch.arange(ws, device=device)[None, None, :, None]
    lc = torch.arange(ws, device=device)[None, None, None, :]
    rr, cc = wr * ws + lr, wc * ws + lc                      # position in the rolled grid
    r0, c0 = (rr + shift) % H, (cc + shift) % W              # original position
    tok = (r0 * W + c0).reshape(nWh * nWw, ws * ws)
    if shift:
        reg = lambda x, n: (x >= n - ws).long() + (x >= n - shift).long()
        lab = (reg(rr, H) * 3 + reg(cc, W)).expand(nWh, nWw, ws, ws).reshape(nWh * nWw, ws * ws)
    else:
        lab = torch.zeros(nWh * nWw, ws * ws, dtype=torch.long, device=device)
    b = torch.arange(B, device=device)[:, None, None] * (H * W)
    tok = (b + tok[None]).reshape(B * nWh * nWw, ws * ws)
    lab = lab[None].expand(B, -1, -1).reshape(B * nWh * nWw, ws * ws)
    i = torch.arange(ws * ws, device=device)
    li, ci = i // ws, i % ws
    rel = (li[:, None] - li[None, :] + ws - 1) * (2 * ws - 1) + (ci[:, None] - ci[None, :] + ws - 1)
    return tok, lab, rel


def qkv_columns(C, heads, layout, device="cpu"):
    """[3, heads, 32] column of q / k / v channel d of head h in the qkv row, per channel layout (WinP.hmajor)."""
    h = torch.arange(heads, device=device)[:, None]
    d = torch.arange(32, device=device)[None, :]
    if layout == 0:
        cols = [h * 32 + d, C + h * 32 + d, 2 * C + h * 32 + d]
    elif layout == 1:
        cols = [h * 96 + d, h * 96 + 32 + d, h * 96 + 64 + d]
    elif layout == 2:
        cols = [h * 32 + d, C + h * 64 + d, C + h * 64 + 32 + d]
    else:
        raise ValueError(layout)
    return torch.stack(cols)


# ------------------------------------------------------------------------------------------------------------ inputs
def _gen(case, device, seed):
    return torch.Generator(device=device).manual_seed(seed + sum(ord(ch) * (i + 1) for i, ch in enumerate(case["name"])) % 100003)


def _spike(x_q, x_k, key_pos, n_keys, first, scale):
    """Plant scores spanning about +-60 along channel 0: q[..., 0] = 16 for every query, k[..., 0] a ramp over the key position whose
    maximum sits on the last key (or the first)."""
    ramp = torch.linspace(-60.0, 60.0, n_keys, device=x_q.device, dtype=torch.float64) / (16 * scale)
    if first:
        ramp = ramp.flip(0)
    r = ramp[key_pos].to(x_k.dtype)
    x_q[..., 0] = 16.0
    x_k[..., 0] = r.reshape(r.shape + (1,) * (x_k.dim() - 1 - r.dim()))


def make_window_inputs(case, device="cuda", seed=0):
    B, H, W, heads, ws, shift, lay = (case[k] for k in ("B", "H", "W", "heads", "ws", "shift", "layout"))
    C, rows = heads * 32, B * H * W
    g = _gen(case, device, seed)
    canon = torch.randn(rows, 3, heads, 32, device=device, generator=g)                     # [token][q k v][head][d]
    tok, lab, rel = window_geometry(B, H, W, ws, shift, device)
    pos = torch.empty(rows, dtype=torch.long, device=device)
    pos[tok.reshape(-1)] = torch.arange(ws * ws, device=device).repeat(tok.shape[0])      # window-local index of each token
    if case["inputs"].startswith("spike"):
        canon[:, 1:, :, 1:] *= 0.25
        canon[:, 0, :, 1:] *= 0.25
        _spike(canon[:, 0], canon[:, 1], pos, ws * ws, case["inputs"] == "spike_first", 32 ** -0.5)
    elif case["inputs"] == "shift_dominant":
        # keys outside the shift region of their window's first token score +60, the others -60: for a query of that region in a
        # border window the -100 mask leaves the masked keys at -40, which still dominate the unmasked ones (-inf would drop them)
        rl = torch.empty(rows, dtype=torch.long, device=device)
        rl[tok.reshape(-1)] = (lab != lab[:, :1]).long().reshape(-1)
        canon[:, :2, :, 1:] *= 0.25
        canon[:, 0, :, 0] = 16.0
        canon[:, 1, :, 0] = torch.where(rl[:, None] != 0, 60.0, -60.0) / (16 * 32 ** -0.5)
    canon = canon.to(torch.bfloat16)
    cols = qkv_columns(C, heads, lay, device)
    qkv = torch.empty(rows, 3 * C, dtype=torch.bfloat16, device=device)
    qkv[:, cols.reshape(-1)] = canon.reshape(rows, -1)
    table = (torch.randn((2 * ws - 1) ** 2, heads, device=device, generator=g) * 0.5).float()
    do = torch.randn(rows, C, device=device, generator=g).to(torch.bfloat16)
    return dict(qkv=qkv, table=table, do=do, cols=cols, tok=tok, lab=lab, rel=rel)


def make_kmask(case, device, g):
    B, Lk, mask = case["B"], case["Lk"], case["mask"]
    if mask == "none":
        return None
    val = FINFO_MIN if mask in ("min", "allmin") else -10000.0
    lens = torch.randint(max(1, Lk // 3), Lk + 1, (B,), device=device, generator=g)
    lens[0] = Lk
    km = (torch.arange(Lk, device=device)[None] >= lens[:, None]).float() * 1.0
    km = torch.where(km > 0, torch.tensor(val, device=device), torch.tensor(0.0, device=device))
    if mask.startswith("all"):
        km[1] = val                                          # sample 1: every key masked
    return km.contiguous()


def make_mha_inputs(case, device="cuda", seed=0):
    B, heads, Lq, Lk, D, ld = (case[k] for k in ("B", "heads", "Lq", "Lk", "D", "ld"))
    C = heads * D
    g = _gen(case, device, seed)
    q = torch.randn(B, Lq, heads, D, device=device, generator=g)
    k = torch.randn(B, Lk, heads, D, device=device, generator=g)
    v = torch.randn(B, Lk, heads, D, device=device, generator=g)
    if case["inputs"].startswith("spike"):
        q[..., 1:] *= 0.25
        k[..., 1:] *= 0.25
        pos = torch.arange(Lk, device=device)[None, :, None].expand(B, Lk, heads)
        _spike(q, k, pos, Lk, case["inputs"] == "spike_first", D ** -0.5)
    do = torch.randn(B, Lq, heads, D, device=device, generator=g)

    def padded(x, ldx):                                      # [B*L, ldx] bf16, the padding NaN (it must never be read)
        buf = torch.full((x.shape[0] * x.shape[1], ldx), float("nan"), dtype=torch.bfloat16, device=device)
        buf[:, :C] = x.reshape(-1, C).to(torch.bfloat16)
        return buf

    inp = dict(q=padded(q, ld["q"]), k=padded(k, ld["k"]), v=padded(v, ld["v"]), do=padded(do, ld["do"]),
               kmask=make_kmask(case, device, g), scale=D ** -0.5, seed=1234 + Lq + Lk)
    return inp


# ------------------------------------------------------------------------------------------------------------ ABI runs
def nan_bf16(rows, cols, device="cuda"):
    return torch.full((rows, cols), NAN_BF16, dtype=torch.int16, device=device).view(torch.bfloat16)


def nan_f32(n, device="cuda"):
    return torch.full((n,), NAN_F32, dtype=torch.int32, device=device).view(torch.float32)


def run_window_fwd(lib, case, inp, lse=True):
    """fiber_window_attn_fwd_bf16 into NaN-filled buffers with one guard row -> (o [rows + 1, C], lse [(rows + 1) * heads])."""
    B, H, W, heads, ws, shift, lay = (case[k] for k in ("B", "H", "W", "heads", "ws", "shift", "layout"))
    C, rows = heads * 32, B * H * W
    o = nan_bf16(rows + 1, C)
    ls = nan_f32((rows + 1) * heads)
    lib.call("fiber_window_attn_fwd_bf16", lib.ptr(inp["qkv"]), lib.ptr(inp["table"]), lib.ptr(o), lib.ptr(ls) if lse else None,
             B, H, W, C, heads, ws, shift, lay)
    return o, ls


def run_window_bwd(lib, case, inp, o, lse, colsum):
    """fiber_window_attn_bwd_bf16 -> (dqkv [rows + 1, 3C], dtable, colsum or None); NaN-filled outputs, one guard row."""
    B, H, W, heads, ws, shift, lay = (case[k] for k in ("B", "H", "W", "heads", "ws", "shift", "layout"))
    C, rows, N = heads * 32, B * H * W, ws * ws
    dqkv = nan_bf16(rows + 1, 3 * C)
    dtab = nan_f32((2 * ws - 1) ** 2 * heads).view(-1, heads)
    delta = nan_f32(rows * heads)
    nz = lib.plain("fiber_window_attn_bwd_slices", rows // N, heads)
    part = nan_f32(nz * heads * N * N)
    cs = cs_ws = None
    if colsum:
        cs_rows = lib.plain("fiber_window_attn_colsum_rows", rows // N, heads, ws)
        assert cs_rows > 0, case["name"]
        cs, cs_ws = nan_f32(3 * C + 1), nan_f32(cs_rows * 3 * C)
    lib.call("fiber_window_attn_bwd_bf16", lib.ptr(inp["qkv"]), lib.ptr(inp["table"]), lib.ptr(o), lib.ptr(inp["do"]), lib.ptr(lse),
             lib.ptr(dqkv), lib.ptr(dtab), lib.ptr(delta), lib.ptr(part), lib.ptr(cs), lib.ptr(cs_ws), B, H, W, C, heads, ws, shift, lay)
    return dqkv, dtab, cs


def mha_entry(case, direction):
    return f"fiber_mha_{'causal_' if case['causal'] else ''}{direction}_bf16"


def run_mha_fwd(lib, case, inp, v=None, lse=True):
    """forward into NaN-filled o [B*Lq + 1, ldo] and lse [B*Lq + 1, heads] (a guard row each)."""
    B, heads, Lq, Lk, D, ld = (case[k] for k in ("B", "heads", "Lq", "Lk", "D", "ld"))
    C = heads * D
    v = inp["v"] if v is None else v
    o = nan_bf16(B * Lq + 1, ld["o"])
    ls = nan_f32((B * Lq + 1) * heads).view(-1, heads)
    lib.call(mha_entry(case, "fwd"), lib.ptr(inp["q"]), lib.ptr(inp["k"]), lib.ptr(v), lib.ptr(inp["kmask"]), lib.ptr(o),
             lib.ptr(ls) if lse else None, B, heads, Lq, Lk, D, ld["q"], ld["k"], v.stride(0), ld["o"], inp["scale"], case["p"],
             inp["seed"], None)
    return o, ls


def run_mha_bwd(lib, case, inp, o, lse):
    """backward into NaN-filled gradients (a guard row each; packed: dq | dk | dv column blocks of one [B*L + 1, ld] buffer)
    -> dict(dq, dk, dv, buf) with dq / dk / dv views of the [B*L, C] parts."""
    B, heads, Lq, Lk, D, ld = (case[k] for k in ("B", "heads", "Lq", "Lk", "D", "ld"))
    C = heads * D
    out = {}
    if case["packed"]:
        buf = nan_bf16(B * Lq + 1, ld["dq"])
        dq, dk, dv = buf[:B * Lq, :C], buf[:B * Lk, C:2 * C], buf[:B * Lk, 2 * C:3 * C]
        out["buf"] = [buf]
    else:
        bq, bk, bv = nan_bf16(B * Lq + 1, ld["dq"]), nan_bf16(B * Lk + 1, ld["dk"]), nan_bf16(B * Lk + 1, ld["dv"])
        dq, dk, dv = bq[:B * Lq, :C], bk[:B * Lk, :C], bv[:B * Lk, :C]
        out["buf"] = [bq, bk, bv]
    delta = nan_f32(B * Lq * heads)
    lib.call(mha_entry(case, "bwd"), lib.ptr(inp["q"]), lib.ptr(inp["k"]), lib.ptr(inp["v"]), lib.ptr(inp["kmask"]), lib.ptr(o),
             lib.ptr(inp["do"]), lib.ptr(lse), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), lib.ptr(delta), B, heads, Lq, Lk, D,
             ld["q"], ld["k"], ld["v"], ld["o"], ld["do"], ld["dq"], ld["dk"], ld["dv"], inp["scale"], case["p"], inp["seed"], None)
    out.update(dq=dq, dk=dk, dv=dv)
    return out


def dropout_keep(lib, case, inp):
    """keep[b, h, i, j] recovered from forwards with one-hot value rows: o[i, head, d] = P[i, j] keep[i, j] / (1 - p) for value row
    j = e_d (D keys per forward); where P underflows the probe cannot see the mask, and the reference does not need it."""
    B, heads, Lq, Lk, D = (case[k] for k in ("B", "heads", "Lq", "Lk", "D"))
    C = heads * D
    keep = torch.zeros(B, heads, Lq, Lk, device=inp["q"].device)
    for c0 in range(0, Lk, D):
        n = min(D, Lk - c0)
        eye = torch.zeros(B, Lk, heads, D, device=inp["q"].device)
        eye[:, c0 + torch.arange(n), :, torch.arange(n)] = 1.0
        o, _ = run_mha_fwd(lib, case, inp, v=eye.reshape(B * Lk, C).to(torch.bfloat16))
        keep[..., c0:c0 + n] = (o[:B * Lq, :C].float().view(B, Lq, heads, D)[..., :n] != 0).permute(0, 2, 1, 3).float()
    return keep


# ------------------------------------------------------------------------------------------------------------ fp64 reference
def attention64(q, k, v, add, do, scale, keep=None, p=0.0, add_mag=None, dtype=torch.float64):
    """softmax(scale q k^T + add) v and its backward in fp64 on [G, H, L, D] operands, with the magnitude terms the bounds need.
    add: [*, *, Lq, Lk] bias + masks (may hold -inf); add_mag: |add| as the kernels hold it (default |add| where finite).
    keep: dropout keep mask (P becomes P * keep / (1 - p)).  dtype: float32 gives the same formulas in fp32 (host check of the bounds)."""
    q, k, v, do = (t.to(dtype) for t in (q, k, v, do))
    add = add.to(dtype)
    raw = scale * q @ k.transpose(-1, -2)
    s = raw + add
    A = scale * q.abs() @ k.abs().transpose(-1, -2)              # score scale: the rounding of the fp32 dot products
    if add_mag is None:
        add_mag = torch.where(torch.isfinite(add), add.abs(), torch.zeros_like(add))
    add_mag = add_mag.to(dtype)
    E = A + raw.abs() + add_mag                                 # E = A + |s| (the mask and bias as the kernels add them)
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    P = e / l
    lse = (m + torch.log(l)).squeeze(-1)
    M = keep.to(dtype) / (1 - p) if keep is not None else torch.ones_like(P)
    Pd = P * M
    O = Pd @ v
    PE = torch.where(P > 0, P * E, torch.zeros_like(P))
    Ebar = PE.sum(-1, keepdim=True)                              # the lse's share of the score rounding
    # O: bf16 store; P (with its dropout factor) rounded to bf16 for the PV MFMA + fp32 accumulation; the score rounding through P
    # (sum_j P_ij dS_ij (M_ij V_j - O_i): the normalisation cancels against O_i)
    o_pv = Pd @ v.abs()
    o_s = torch.zeros_like(O)
    for d0 in range(0, O.shape[-1], 8):
        o_s[..., d0:d0 + 8] = (PE[..., None] * (M[..., None] * v[..., None, :, d0:d0 + 8] - O[..., None, d0:d0 + 8]).abs()).sum(-2)
    dV = Pd.transpose(-1, -2) @ do
    dP = do @ v.transpose(-1, -2)
    delta = (do * O).sum(-1, keepdim=True)
    dS = P * (M * dP - delta)
    R = P * (M * (do.abs() @ v.abs().transpose(-1, -2)) + (do * O).abs().sum(-1, keepdim=True))
    RE = R * (E + Ebar)
    dQ = scale * dS @ k
    dK = scale * dS.transpose(-1, -2) @ q
    out = dict(O=O, lse=lse, dQ=dQ, dK=dK, dV=dV, dS=dS, P=P)
    terms = dict(
        O=(U * O.abs() + TINY, dict(C_PV=o_pv, C_S=o_s)),
        lse=(2.0 ** -22 * lse.abs(), dict(C_S=Ebar.squeeze(-1))),
        dV=(U * dV.abs() + TINY, dict(C_PV=Pd.abs().transpose(-1, -2) @ do.abs(), C_S=(Pd * (E + Ebar)).transpose(-1, -2) @ do.abs())),
        dQ=(U * dQ.abs() + TINY, dict(C_DS=scale * R @ k.abs(), C_S=scale * RE @ k.abs())),
        dK=(U * dK.abs() + TINY, dict(C_DS=scale * R.transpose(-1, -2) @ q.abs(), C_S=scale * RE.transpose(-1, -2) @ q.abs())),
        dS=(torch.full_like(dS, TINY), dict(C_DS=R, C_S=RE)),
    )
    return out, terms


def _blocks(G, per, limit=1 << 24):
    step = max(1, limit // max(1, per))
    return [(i, min(G, i + step)) for i in range(0, G, step)]


def window_reference(case, inp, mask_value=-100.0, dtype=torch.float64):
    """fp64 reference of a window case in canonical form [G, heads, N, 32]; dbias_table by scatter-add of dS over windows and (i, j).
    Returns (ref, terms) with dqkv / o as [rows, 3, heads, 32] / [rows, heads, 32], dtable [(2ws-1)^2, heads]."""
    B, H, W, heads, ws, shift = (case[k] for k in ("B", "H", "W", "heads", "ws", "shift"))
    N, rows = ws * ws, B * H * W
    tok, lab, rel = inp["tok"], inp["lab"], inp["rel"]
    G, nW = tok.shape[0], (H // ws) * (W // ws)
    dev = inp["qkv"].device
    canon = inp["qkv"][:, inp["cols"].reshape(-1)].view(rows, 3, heads, 32).to(torch.float64)
    do = inp["do"].view(rows, heads, 32).to(torch.float64)
    bias = inp["table"].to(torch.float64)[rel.reshape(-1)].view(N, N, heads).permute(2, 0, 1)      # [heads, N, N]
    ref = {k: torch.zeros(rows, heads, 32, dtype=torch.float64, device=dev) for k in ("o", "dq", "dk", "dv")}
    trm = {}
    nt = (2 * ws - 1) ** 2
    dtab = torch.zeros(nt, heads, dtype=torch.float64, device=dev)
    dtab_b = {c: torch.zeros(nt, heads, dtype=torch.float64, device=dev) for c in ("C_DS", "C_S")}
    dtab_abs = torch.zeros(nt, heads, dtype=torch.float64, device=dev)
    for g0, g1 in _blocks(G, heads * N * N * 32):
        t = tok[g0:g1]
        qg = canon[t][:, :, 0].permute(0, 2, 1, 3)             # [g, heads, N, 32]
        kg = canon[t][:, :, 1].permute(0, 2, 1, 3)
        vg = canon[t][:, :, 2].permute(0, 2, 1, 3)
        dog = do[t].permute(0, 2, 1, 3)
        add = bias[None].expand(g1 - g0, -1, -1, -1)
        mag = add.abs()
        if shift:
            lb = lab[g0:g1]
            msk = torch.where(lb[:, :, None] != lb[:, None, :], mask_value, 0.0).to(torch.float64)[:, None]
            add = add + msk
            mag = mag + torch.where(torch.isfinite(msk), msk.abs(), torch.zeros_like(msk))
        out, terms = attention64(qg, kg, vg, add, dog, 32 ** -0.5, add_mag=mag, dtype=dtype)
        for key, name in (("o", "O"), ("dq", "dQ"), ("dk", "dK"), ("dv", "dV")):
            ref[key][t.reshape(-1)] = out[name].double().permute(0, 2, 1, 3).reshape(-1, heads, 32)
            base, tt = terms[name]
            if key not in trm:
                trm[key] = (torch.zeros_like(ref[key]), {c: torch.zeros_like(ref[key]) for c in tt})
            trm[key][0][t.reshape(-1)] = base.double().permute(0, 2, 1, 3).reshape(-1, heads, 32)
            for c, x in tt.items():
                trm[key][1][c][t.reshape(-1)] = x.double().permute(0, 2, 1, 3).reshape(-1, heads, 32)
        idx = rel.reshape(-1)
        dS = out["dS"].double()
        dtab.index_add_(0, idx, dS.sum(0).permute(1, 2, 0).reshape(N * N, heads))
        dtab_abs.index_add_(0, idx, dS.abs().sum(0).permute(1, 2, 0).reshape(N * N, heads))
        for c, x in terms["dS"][1].items():
            dtab_b[c].index_add_(0, idx, x.double().sum(0).permute(1, 2, 0).reshape(N * N, heads))
    ref["dtable"] = dtab
    # dbias_table: the per-entry dS terms scatter-added, the fp32 sums over windows (C_SUM of sum |dS|) and the fp32 result
    trm["dtable"] = (2.0 ** -22 * dtab.abs() + TINY, dict(dtab_b, C_SUM=dtab_abs))
    return ref, trm


def mha_reference(case, inp, keep=None):
    """fp64 reference of an mha / causal case in canonical form [B, heads, L, D]."""
    B, heads, Lq, Lk, D = (case[k] for k in ("B", "heads", "Lq", "Lk", "D"))
    C = heads * D
    cv = lambda x, L: x[:, :C].to(torch.float64).view(B, L, heads, D).permute(0, 2, 1, 3)
    q, k, v, do = cv(inp["q"], Lq), cv(inp["k"], Lk), cv(inp["v"], Lk), cv(inp["do"], Lq)
    dev = q.device
    add = torch.zeros(B, 1, Lq, Lk, dtype=torch.float64, device=dev)
    mag = torch.zeros_like(add)
    km = inp["kmask"]
    if km is not None:
        km = km.to(torch.float64)[:, None, None, :]
        add = add + km
        # a finfo.min key's score is KMASK_SCORE in the kernels: that magnitude is what an fp32 lse of a wholly masked row rounds
        mag = mag + torch.where(km > FINFO_MIN, km.abs(), torch.full_like(km, KMASK_SCORE_NAT))
    if case["causal"]:
        i = torch.arange(Lq, device=dev)
        add = add + torch.where(i[None, :] > i[:, None], -math.inf, 0.0).to(torch.float64)
    out, terms = attention64(q, k, v, add, do, inp["scale"], keep=keep, p=case["p"], add_mag=mag.expand_as(add))
    return out, terms
