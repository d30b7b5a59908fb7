"""Every element-wise, cross-entropy and embedding kernel path, element by element against fp64 (tests/ew_cases.py: the hash
restatement, the references, the bounds).

Each case runs the C ABI directly with every output NaN-filled and GUARD elements (rows) after it: every owned element must be
written and no guard may change (workspaces included).  Dropout and DropPath masks must match the host restatement exactly.  Two
runs of every case are bit-for-bit equal -- d alpha, the dot product and the five embedding gradient tables included (fixed-order
folds and segment sums).  FIBER_EW_CALIBRATE=<file> writes, per constant of
ew_cases.CONST, the largest value any element needed."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

from tests import ew_cases as ec
from tests.hip_util import BF, DEV, assert_elementwise
from tests.mp_util import run_bounded

pytestmark = pytest.mark.gpu

CONST = ec.CONST
_CAL = os.environ.get("FIBER_EW_CALIBRATE")
_needed = {}
G = 64                                                       # guard elements after every output


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from fiber_amd import lib
    lib.load()
    return lib


def rc(lib, name, *args):
    return getattr(lib.load(), name)(*args, torch.cuda.current_stream().cuda_stream)


def check(name, got, ref, base, terms):
    """assert_elementwise with bound = base + sum_c CONST[c] * terms[c] (2-D views: [n] -> [n, 1])"""
    fix = (lambda t: t[:, None] if torch.is_tensor(t) and t.dim() == 1 else t)
    got, ref, base = fix(got.detach().double()), fix(ref.double()), fix(base)
    terms = {c: fix(t.double()) for c, t in terms.items()}
    bound = base + sum(CONST[c] * t for c, t in terms.items())
    if _CAL:
        err = (got - ref).abs()
        for c, t in terms.items():
            rest = base + sum(CONST[o] * x for o, x in terms.items() if o != c)
            need = ((err - rest) / t.clamp_min(1e-300)).where(t > 0, torch.zeros_like(err)).max().item()
            if need > _needed.get(c, (0.0, ""))[0]:
                _needed[c] = (need, name, math.log2(need) if need > 0 else None)
        with open(_CAL, "w") as f:
            json.dump(_needed, f, indent=1)
    return assert_elementwise(name, got, ref, bound)


def nan_buf(n, dtype, rows=None):
    shape = (n + G,) if rows is None else (n + 1, rows)
    if dtype == BF:
        return torch.full(shape, ec.NAN_BF16, dtype=torch.int16, device=DEV).view(BF)
    if dtype == torch.float32:
        return torch.full(shape, ec.NAN_F32, dtype=torch.int32, device=DEV).view(torch.float32)
    return torch.full(shape, -7, dtype=dtype, device=DEV)


def bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32) if t.element_size() == 4 else t


def isnan_bits(t):
    return bits(t) == (ec.NAN_BF16 if t.dtype == BF else ec.NAN_F32)


def assert_written(name, buf, n):
    flat = buf.reshape(-1) if buf.dim() == 1 else buf
    missed = int(isnan_bits(flat[:n]).sum())
    stray = int((~isnan_bits(flat[n:])).sum())
    assert missed == 0, f"{name}: {missed} owned elements never written"
    assert stray == 0, f"{name}: {stray} guard elements written"


def same(name, a, b):
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), f"{name}: {k} differs between two runs"


def P(lib, t):
    return lib.ptr(t)


def rnd(n, seed, scale=1.0, dtype=BF):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(n, device=DEV, generator=g) * scale).to(dtype)


SEED_BASE_VAL = 0x5_0000_0000
SEED_BASE = torch.tensor([SEED_BASE_VAL], dtype=torch.int64, device=DEV) if torch.cuda.is_available() else None


# ---- stream add, forward -------------------------------------------------------------------------------------------------------------
WRAP = 8 * 2048 * 256                                        # one grid-stride round of the 2048-workgroup element-wise kernels
SA_FWD = [  # (name, res_kind, b, alpha, rowscale per_sample, p_a, p_b, outs, n)
    ("none_a_only_16", 0, False, False, 0, 0.0, 0.0, "16", 8),
    ("bf16_b_alpha_both", 1, True, True, 0, 0.0, 0.0, "both", 8 * 1000),
    ("f32_b_rs_drop_both", 2, True, True, 8 * 37, 0.1, 0.1, "both", WRAP + 8 * 61),
    ("f32_b_noalpha_32", 2, True, False, 0, 0.0, 0.5, "32", 8 * 4097),
    ("bf16_pa_rs_16", 1, False, False, 8 * 3, 0.999, 0.0, "16", 8 * 999),
    ("none_b_alpha_rs", 0, True, True, 512 * 576 // 64 * 8, 0.1, 0.0, "both", 32 * 576 * 512),
]


@pytest.mark.parametrize("case", SA_FWD, ids=[c[0] for c in SA_FWD])
def test_stream_add_fwd(lib, case):
    name, kind, has_b, has_alpha, per, p_a, p_b, outs, n = case
    a, b = rnd(n, 1), (rnd(n, 2) if has_b else None)
    res = None if kind == 0 else rnd(n, 3, 4.0, BF if kind == 1 else torch.float32)
    alpha = torch.tensor([-0.625], device=DEV) if has_alpha else None
    rs = None
    if per:
        ns = -(-n // per)
        rs = torch.where(torch.arange(ns, device=DEV) % 3 == 1, 0.0, 1.0 / 0.9).float()
    seed_a, seed_b = 0x1234_5678_9ABC, 0x42
    base = SEED_BASE if p_b > 0 else None                    # the device-resident per-step part of the keys (graph replay)

    def run():
        o32 = nan_buf(n, torch.float32) if outs in ("32", "both") else None
        o16 = nan_buf(n, BF) if outs in ("16", "both") else None
        assert rc(lib, "fiber_stream_add", P(lib, res), kind, P(lib, a), P(lib, b), P(lib, alpha), P(lib, rs), per, p_a, seed_a, p_b,
                  seed_b, P(lib, base), P(lib, o32), P(lib, o16), n) == 0
        return {k: v for k, v in (("o32", o32), ("o16", o16)) if v is not None}
    r1, r2 = run(), run()
    same(name, r1, r2)
    rs_e = rs.double().repeat_interleave(per)[:n] if rs is not None else None
    if base is not None:
        seed_a, seed_b = seed_a + SEED_BASE_VAL, seed_b + SEED_BASE_VAL
    ref, term = ec.stream_add_ref(res, a, b, None if alpha is None else alpha.item(), rs_e, p_a, seed_a, p_b, seed_b)
    for k, v in r1.items():
        assert_written(f"{name} {k}", v, n)
        base = ec.BF16_STORE * ref.abs() if k == "o16" else torch.zeros_like(ref)
        check(f"{name} {k}", v[:n], ref, base, {"EW": term})
    if p_a > 0:                                              # the masked elements are exact zeros (res absent, b absent there)
        m = ec.mask_t(seed_a, n, p_a, DEV)
        if kind == 0 and not has_b:
            assert torch.equal(r1["o16"][:n][~m].float(), torch.zeros(int((~m).sum()), device=DEV))


# ---- stream add, backward ------------------------------------------------------------------------------------------------------------
BWD_BIG = 8 * (512 * 256 * 4 + 12345)                        # leaves the U = 4 loop ragged at the 512-workgroup d alpha grid
SA_BWD = [  # (name, da, db, dalpha, per, p_a, p_b, n)
    ("da_only", True, False, False, 0, 0.1, 0.0, 8 * 333),
    ("db_only_rs", False, True, False, 8 * 5, 0.0, 0.1, 8 * 1000),
    ("db_dalpha", False, True, True, 0, 0.0, 0.0, 8),
    ("all_masks_rs", True, True, True, 8 * 37, 0.1, 0.5, BWD_BIG),
    ("all_plain", True, True, True, 0, 0.0, 0.0, WRAP + 8 * 3),
    ("stage2", True, True, True, 576 * 512, 0.0, 0.1, 32 * 576 * 512),
]


@pytest.mark.parametrize("case", SA_BWD, ids=[c[0] for c in SA_BWD])
def test_stream_add_bwd(lib, case):
    name, want_da, want_db, want_dal, per, p_a, p_b, n = case
    dy, b = rnd(n, 4), rnd(n, 5)
    alpha = torch.tensor([0.375], device=DEV)
    rs = None
    if per:
        rs = torch.where(torch.arange(-(-n // per), device=DEV) % 4 == 2, 0.0, 1.25).float()
    sa, sb = 77, (1 << 63) + 5
    base = SEED_BASE if p_b > 0 else None

    def run():
        da = nan_buf(n, BF) if want_da else None
        db = nan_buf(n, BF) if want_db else None
        dal = nan_buf(1, torch.float32) if want_dal else None
        ws = nan_buf(512, torch.float32) if want_dal else None
        assert rc(lib, "fiber_stream_add_bwd", P(lib, dy), P(lib, b), P(lib, alpha), P(lib, rs), per, p_a, sa, p_b, sb, P(lib, base),
                  P(lib, da), P(lib, db), P(lib, dal), P(lib, ws), n) == 0
        out = {k: v for k, v in (("da", da), ("db", db), ("dalpha", dal)) if v is not None}
        if ws is not None:
            assert not bool((~isnan_bits(ws[512:])).any()), f"{name}: written past the workspace"
        return out
    r1, r2 = run(), run()
    same(name, r1, r2)
    if base is not None:
        sa, sb = (sa + SEED_BASE_VAL) & ((1 << 64) - 1), (sb + SEED_BASE_VAL) & ((1 << 64) - 1)
    g = dy.double()
    if rs is not None:
        g = g * rs.double().repeat_interleave(per)[:n]
    ma = ec.mask_t(sa, n, p_a, DEV) if p_a > 0 else None
    mb = ec.mask_t(sb, n, p_b, DEV) if p_b > 0 else None
    if want_da:
        ref = g if ma is None else torch.where(ma, g * ec.inv_keep(p_a), torch.zeros_like(g))
        assert_written(f"{name} da", r1["da"], n)
        check(f"{name} da", r1["da"][:n], ref, ec.BF16_STORE * ref.abs(), {"EW": ref.abs()})
    if want_db:
        m = torch.ones_like(g) if mb is None else torch.where(mb, ec.inv_keep(p_b), 0.0).double()
        ref = 0.375 * m * g
        assert_written(f"{name} db", r1["db"], n)
        check(f"{name} db", r1["db"][:n], ref, ec.BF16_STORE * ref.abs(), {"EW": ref.abs()})
        if want_dal:
            t = g * m * b.double()
            assert_written(f"{name} dalpha", r1["dalpha"], 1)
            check(f"{name} dalpha", r1["dalpha"][:1], t.sum()[None], torch.zeros(1, device=DEV, dtype=torch.float64),
                  {"SUM": t.abs().sum()[None]})


# ---- single-pass kernels -------------------------------------------------------------------------------------------------------------
SIZES = [8, WRAP + 8 * 77, 32 * 576 * 512]


def _gelu_grad64(h):
    h = h.double()
    return 0.5 * (1 + torch.erf(h / math.sqrt(2))) + h * torch.exp(-0.5 * h * h) / math.sqrt(2 * math.pi)


@pytest.mark.parametrize("n", SIZES)
def test_single_pass_kernels(lib, n):
    x, y = rnd(n, 6, 2.0), rnd(n, 7, 3.0)
    alpha = torch.tensor([-1.5], device=DEV)
    # scale_add: a / alpha NULL or not, mult != 1
    for has_a, has_al, mult in ((True, True, 1.0), (False, True, 0.5), (True, False, -2.0), (False, False, 3.0)):
        outs = []
        for _ in range(2):
            o = nan_buf(n, BF)
            assert rc(lib, "fiber_scale_add_bf16", P(lib, x) if has_a else None, P(lib, y), P(lib, alpha) if has_al else None, mult,
                      P(lib, o), n) == 0
            outs.append(o)
        assert torch.equal(bits(outs[0]), bits(outs[1]))
        s = (-1.5 if has_al else 1.0) * float(np.float32(mult))
        ref = (x.double() if has_a else 0) + s * y.double()
        term = (x.double().abs() if has_a else 0) + abs(s) * y.double().abs()
        assert_written(f"scale_add {n}", outs[0], n)
        check(f"scale_add {n} a={has_a} alpha={has_al} mult={mult}", outs[0][:n], ref, ec.BF16_STORE * ref.abs(), {"EW": term})
    # rowscale_add, r NULL or not
    per = 8 * 9 if n > 8 else 8
    sc = torch.where(torch.arange(-(-n // per), device=DEV) % 5 == 0, 0.0, 1.0 / 0.8).float()
    for has_r in (True, False):
        o = nan_buf(n, BF)
        assert rc(lib, "fiber_rowscale_add_bf16", P(lib, x) if has_r else None, P(lib, y), P(lib, sc), P(lib, o), n, per) == 0
        se = sc.double().repeat_interleave(per)[:n]
        ref = (x.double() if has_r else 0) + se * y.double()
        assert_written(f"rowscale_add {n}", o, n)
        check(f"rowscale_add {n} r={has_r}", o[:n], ref, ec.BF16_STORE * ref.abs(), {"EW": ref.abs() + se * y.double().abs()})
    # dropout: the mask must be the restated one, element by element
    base = torch.tensor([0x0123_4567_0000_0000], dtype=torch.int64, device=DEV)
    for p, sbase in ((0.0, False), (0.1, False), (0.5, True), (0.999, False)):
        o = nan_buf(n, BF)
        assert rc(lib, "fiber_dropout_bf16", P(lib, x), P(lib, o), n, p, 99, P(lib, base) if sbase else None) == 0
        key = (99 + (0x0123_4567_0000_0000 if sbase else 0)) & ((1 << 64) - 1)
        m = ec.mask_t(key, n, p, DEV)
        ref = torch.where(m, x.double() * ec.inv_keep(p), torch.zeros_like(x.double()))
        assert_written(f"dropout {n}", o, n)
        kept = o[:n] != 0
        assert torch.equal(kept | (x == 0), m | (x == 0)), f"dropout p={p} n={n}: mask differs from the restatement"
        check(f"dropout {n} p={p}", o[:n], ref, ec.BF16_STORE * ref.abs(), {"EW": ref.abs()})
    # gelu_bwd
    o = nan_buf(n, BF)
    assert rc(lib, "fiber_gelu_bwd_bf16", P(lib, y), P(lib, x), P(lib, o), n) == 0
    ref = y.double() * _gelu_grad64(x)
    assert_written(f"gelu_bwd {n}", o, n)
    check(f"gelu_bwd {n}", o[:n], ref, ec.BF16_STORE * ref.abs() + ec.GELU_BWD_ERR * y.double().abs(), {"EW": ref.abs()})
    # cast: bitwise the torch rounding
    x32 = rnd(n, 8, 100.0, torch.float32)
    o = nan_buf(n, BF)
    assert rc(lib, "fiber_cast_f32_bf16", P(lib, x32), P(lib, o), n) == 0
    assert_written(f"cast {n}", o, n)
    assert torch.equal(bits(o[:n]), bits(x32.to(BF)))


def test_droppath_scale(lib):
    """bit for bit floor(keep + u) / keep of the restated draw; keep = 1 on a seed whose draw reaches h >= 2^32 - 128 gives 1, not 2"""
    seed = 208044                                            # sample 50 draws h >= 2^32 - 128 (ec.seed_hitting_top)
    base = torch.tensor([1 << 40], dtype=torch.int64, device=DEV)
    for n, keep, s, sbase in ((1000, 1.0, seed, False), (1000, 0.9, 5, False), (64, 0.75, 9, True), (1, 0.5, 3, False)):
        o = nan_buf(n, torch.float32)
        assert rc(lib, "fiber_droppath_scale_f32", P(lib, o), n, keep, s, P(lib, base) if sbase else None) == 0
        assert_written(f"droppath {n}", o, n)
        want = torch.from_numpy(ec.droppath_scale(n, keep, s + ((1 << 40) if sbase else 0))).to(DEV)
        assert torch.equal(bits(o[:n]), bits(want)), (n, keep)


# ---- column sums, fold, dot ---------------------------------------------------------------------------------------------------------
COLSUM = [(1, 8, 8), (7, 24, 32), (511, 264, 264), (1000, 1000, 1024), (4099, 2056, 2056), (300001, 128, 128), (70001, 768, 776)]


@pytest.mark.parametrize("M,N,ld", COLSUM, ids=[f"{m}x{n}_ld{l}" for m, n, l in COLSUM])
def test_colsums(lib, M, N, ld):
    slabs = lib.load().fiber_colsum_slabs(M, N)
    x = rnd(M * ld, 10, 1.0).view(M, ld)
    xs = x[:, :N]
    ref, term = ec.colsum_ref(xs)

    def run(fn, make_args):
        out, ws = nan_buf(N, torch.float32), nan_buf(slabs * N, torch.float32)
        assert rc(lib, fn, *make_args(out, ws)) == 0
        assert not bool((~isnan_bits(ws[slabs * N:])).any()), f"{fn}: written past the workspace"
        return out
    o1 = run("fiber_colsum_bf16", lambda o, w: (P(lib, x), P(lib, o), P(lib, w), M, N, ld))
    o2 = run("fiber_colsum_bf16", lambda o, w: (P(lib, x), P(lib, o), P(lib, w), M, N, ld))
    assert torch.equal(bits(o1), bits(o2))
    assert_written(f"colsum {M}x{N}", o1, N)
    check(f"colsum {M}x{N} ld {ld} ({slabs} slabs)", o1[:N], ref, torch.zeros_like(ref), {"SUM": term})
    if ld != N:
        return
    h = rnd(M * N, 11, 2.0).view(M, N)
    dh = nan_buf(M * N, BF)
    o = run("fiber_gelu_bwd_colsum_bf16", lambda o, w: (P(lib, x), P(lib, h), P(lib, dh), P(lib, o), P(lib, w), M, N))
    assert_written("gelu_bwd_colsum dh", dh, M * N)
    dref = x.double() * _gelu_grad64(h)
    check(f"gelu_bwd_colsum dh {M}x{N}", dh[:M * N].view(M, N), dref, ec.BF16_STORE * dref.abs() + ec.GELU_BWD_ERR * x.double().abs(),
          {"EW": dref.abs()})
    r2, t2 = ec.colsum_ref(dh[:M * N].view(M, N))               # the column sums of what the kernel stored
    check(f"gelu_bwd_colsum db {M}x{N}", o[:N], r2, torch.zeros_like(r2), {"SUM": t2})
    rps = 7 if M > 7 else 1                                     # does not divide the slab height; every third sample scale is 0
    sc = torch.where(torch.arange(-(-M // rps), device=DEV) % 3 == 0, 0.0, 1.0 / 0.9).float()
    y = nan_buf(M * N, BF)
    o = run("fiber_rowscale_colsum_bf16", lambda o, w: (P(lib, x), P(lib, sc), P(lib, y), P(lib, o), P(lib, w), M, N, rps))
    assert_written("rowscale_colsum y", y, M * N)
    yref = x.double() * sc.double().repeat_interleave(rps)[:M, None]
    check(f"rowscale_colsum y {M}x{N}", y[:M * N].view(M, N), yref, ec.BF16_STORE * yref.abs(), {"EW": yref.abs()})
    r3, t3 = ec.colsum_ref(y[:M * N].view(M, N))
    check(f"rowscale_colsum db {M}x{N}", o[:N], r3, torch.zeros_like(r3), {"SUM": t3})


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 48, 49, 64, 65, 512])
def test_fold_rows(lib, rows):
    for N in (1, 15, 16, 17, 50265):
        part = rnd(rows * N, rows * 7 + N, 1.0, torch.float32).view(rows, N)
        outs = []
        for _ in range(2):
            o = nan_buf(N, torch.float32)
            assert rc(lib, "fiber_fold_rows_f32", P(lib, part), P(lib, o), rows, N) == 0
            outs.append(o)
        assert torch.equal(bits(outs[0]), bits(outs[1]))
        assert_written(f"fold {rows}x{N}", outs[0], N)
        ref, term = ec.colsum_ref(part)
        check(f"fold {rows}x{N}", outs[0][:N], ref, torch.zeros_like(ref), {"SUM": term})


@pytest.mark.parametrize("n", [8, 8 * 3001, 8 * 512 * 256 * 3 + 8 * 5])
def test_dot(lib, n):
    a, b = rnd(n, 12), rnd(n, 13)
    outs = []
    for _ in range(2):
        o, ws = nan_buf(1, torch.float32), nan_buf(512, torch.float32)
        assert rc(lib, "fiber_dot_bf16", P(lib, a), P(lib, b), P(lib, o), P(lib, ws), n) == 0
        assert not bool((~isnan_bits(ws[512:])).any())
        outs.append(o)
    assert torch.equal(bits(outs[0]), bits(outs[1])), "dot: two runs differ"
    assert_written("dot", outs[0], 1)
    t = a.double() * b.double()
    check(f"dot {n}", outs[0][:1], t.sum()[None], torch.zeros(1, dtype=torch.float64, device=DEV), {"SUM": t.abs().sum()[None]})


# ---- cross-entropy --------------------------------------------------------------------------------------------------------------------
CE = [(17, 24, -100), (1000, 40, -100), (50265, 1280, -100), (50265, 16, 7), (1001, 8, -100)]


def _ce_inputs(V, rows, ignore):
    g = torch.Generator(device=DEV).manual_seed(V + rows)
    x = (torch.randn(rows, V, device=DEV, generator=g) * 3).to(BF)
    x[1] *= 40                                                # a wide bf16 range
    x[2] = (x[2].float() * 1e-3).to(BF)
    lab = torch.randint(0, V, (rows,), device=DEV, generator=g)
    head = [(8 - (r * V) % 8) % 8 for r in range(rows)]
    for r in range(rows):                                     # labels at 0, in the head, first / last vector, tail, V - 1
        k = r % 7
        nvec = (V - head[r]) // 8
        lab[r] = [0, max(head[r] - 1, 0), head[r], head[r] + 8 * nvec - 1, min(head[r] + 8 * nvec, V - 1), V - 1, lab[r].item()][k]
    ign = torch.arange(rows, device=DEV) % 5 == 3
    lab[ign] = ignore
    if rows == 8:
        lab[:] = ignore                                       # all rows ignored
    # ties of the maximum in the head, a vector, the tail and across waves
    for r in range(min(rows, 12)):
        m = x[r].float().abs().max().item() * 2 + 1
        spots = [[0, V // 2], [head[r] + 3, V - 1], [V - 1, V - 2], [8 * 70 + head[r], 8 * 3 + head[r]]][r % 4]
        for j in spots:
            if j < V:
                x[r, j] = m
    return x, lab


@pytest.mark.parametrize("V,rows,ignore", CE, ids=[f"V{v}_r{r}_ig{i}" for v, r, i in CE])
def test_cross_entropy(lib, V, rows, ignore):
    x, lab = _ce_inputs(V, rows, ignore)

    def fwd():
        loss, lse, pred = nan_buf(rows, torch.float32), nan_buf(rows, torch.float32), nan_buf(rows, torch.int32)
        assert rc(lib, "fiber_ce_fwd_bf16", P(lib, x), P(lib, lab), P(lib, loss), P(lib, lse), P(lib, pred), rows, V, ignore) == 0
        return dict(loss=loss, lse=lse, pred=pred)
    f1, f2 = fwd(), fwd()
    same("ce fwd", f1, f2)
    assert_written("ce loss", f1["loss"], rows)
    assert_written("ce lse", f1["lse"], rows)
    assert torch.all(f1["pred"][rows:] == -7), "ce pred: guard written"
    lse, loss, pred, picked = ec.ce_ref(x, lab, ignore)
    ign = lab == ignore
    assert torch.equal(f1["pred"][:rows].long(), pred), "pred differs from torch.argmax (-1 on ignored rows)"
    assert bool((f1["loss"][:rows][ign] == 0).all()) and bool((f1["lse"][:rows][ign] == 0).all())
    lse0 = torch.where(ign, torch.zeros_like(lse), lse)
    z = torch.zeros_like(lse)
    check(f"ce lse V{V}", f1["lse"][:rows], lse0, z, {"LSE": torch.where(ign, z, 1 + lse.abs())})
    check(f"ce loss V{V}", f1["loss"][:rows], loss, z, {"LSE": torch.where(ign, z, 1 + lse.abs() + picked.abs())})
    scale = torch.tensor([1.0 / max(1, int((~ign).sum()))], device=DEV)

    def bwd():
        dx = nan_buf(rows * V, BF)
        assert rc(lib, "fiber_ce_bwd_bf16", P(lib, x), P(lib, lab), P(lib, f1["lse"]), P(lib, scale), P(lib, dx), rows, V, ignore) == 0
        return dict(dx=dx)
    b1, b2 = bwd(), bwd()
    same("ce bwd", b1, b2)
    assert_written("ce dx", b1["dx"], rows * V)
    ref, p = ec.ce_bwd_ref(x, lab, f1["lse"][:rows], scale.item(), ignore)
    dx = b1["dx"][:rows * V].view(rows, V)
    assert bool((dx[ign] == 0).all()), "ignored rows must be exact zeros"
    check(f"ce dx V{V}", dx, ref, ec.BF16_STORE * ref.abs() + ec.EXP_FLOOR * scale.item(),
          {"EXP": p * (1 + x.double().abs() + f1["lse"][:rows].double().abs()[:, None]) * scale.item()})
    # labelled column sums of the gradient
    slabs = lib.load().fiber_colsum_labelled_slabs(rows)
    o, ws = nan_buf(V, torch.float32), nan_buf(slabs * V, torch.float32)
    assert rc(lib, "fiber_colsum_labelled_bf16", P(lib, dx), P(lib, lab), P(lib, o), P(lib, ws), rows, V, ignore) == 0
    assert_written("colsum_labelled", o, V)
    r, t = ec.colsum_ref(dx[~ign]) if bool((~ign).any()) else (torch.zeros(V, dtype=torch.float64, device=DEV),) * 2
    check(f"colsum_labelled V{V}", o[:V], r, torch.zeros_like(r), {"SUM": t})


@pytest.mark.parametrize("rows", [511, 512, 4095, 4096, 122880])
def test_colsum_labelled_slabs(lib, rows):
    """slabs 1 / 4 / 8 at their edges, V not a multiple of 256, a slab without a labelled row; 122880 rows is the largest the LDS list takes"""
    V, ignore = 264, -100
    slabs = lib.load().fiber_colsum_labelled_slabs(rows)
    x = rnd(rows * V, rows, 1.0).view(rows, V)
    lab = torch.where(torch.arange(rows, device=DEV) % 3 == 0, 5, ignore).long()
    lab[: -(-rows // slabs)] = ignore                          # the first slab has no labelled row
    outs = []
    for _ in range(2):
        o, ws = nan_buf(V, torch.float32), nan_buf(slabs * V, torch.float32)
        assert rc(lib, "fiber_colsum_labelled_bf16", P(lib, x), P(lib, lab), P(lib, o), P(lib, ws), rows, V, ignore) == 0
        outs.append(o)
    assert torch.equal(bits(outs[0]), bits(outs[1]))
    assert_written("colsum_labelled", outs[0], V)
    r, t = ec.colsum_ref(x[lab != ignore])
    check(f"colsum_labelled {rows}", outs[0][:V], r, torch.zeros_like(r), {"SUM": t})
    if rows == 122880:
        o = nan_buf(V, torch.float32)
        x2 = rnd(122881 * 24, 1, 1.0)
        l2 = torch.full((122881,), ignore, dtype=torch.int64, device=DEV)
        assert rc(lib, "fiber_colsum_labelled_bf16", P(lib, x2), P(lib, l2), P(lib, o), P(lib, ws), 122881, 24, ignore) == 1


# ---- RoBERTa embeddings ---------------------------------------------------------------------------------------------------------------
EMB = [(4, 40, 0.0, 6), (128, 1, 0.1, 6), (256, 40, 0.0, 6), (260, 40, 0.1, 6), (768, 40, 0.1, 6), (1024, 512, 0.0, 6), (2048, 40, 0.0, 6),
       (768, 40, 0.1, 96)]                                    # 96 samples: position and <s> segments longer than 32 rows


@pytest.mark.parametrize("C,S,p,B", EMB, ids=[f"C{c}_S{s}_p{p}_B{b}" for c, s, p, b in EMB])
def test_roberta_embed(lib, C, S, p, B):
    pad, Vw, eps = 1, 300, 1e-5
    g = torch.Generator(device=DEV).manual_seed(C + S)
    ids = torch.randint(3, Vw, (B, S), device=DEV, generator=g)
    if S > 1:
        ids[0, S // 2:] = pad                                  # pads at the end, the middle and the start of a row
        ids[1, S // 3] = pad
        ids[2, 0] = pad
        ids[3, :] = pad                                        # an all-pad row
        ids[4, :] = 7                                          # one id in every position of a row
        ids[ids[:, 1] != pad, 1] = 9                           # and one id shared by every sample
    ids[:, 0] = torch.where(ids[:, 0] == pad, ids[:, 0], torch.zeros_like(ids[:, 0]))   # <s> in most rows
    word = torch.randn(Vw, C, device=DEV, generator=g)
    pos_tab = torch.randn(S + 2, C, device=DEV, generator=g) * 0.5
    type_tab = torch.randn(2, C, device=DEV, generator=g) * 0.1
    gamma = 1 + 0.2 * torch.randn(C, device=DEV, generator=g)
    beta = 0.1 * torch.randn(C, device=DEV, generator=g)
    rows, seed = B * S, 0xE111

    def fwd():
        y, pos = nan_buf(rows * C, BF), nan_buf(rows, torch.int32)
        mean, rstd = nan_buf(rows, torch.float32), nan_buf(rows, torch.float32)
        assert rc(lib, "fiber_roberta_embed_fwd", P(lib, ids), P(lib, word), P(lib, pos_tab), P(lib, type_tab), P(lib, gamma), P(lib, beta),
                  P(lib, y), P(lib, pos), P(lib, mean), P(lib, rstd), B, S, C, pad, eps, p, seed, None) == 0
        return dict(y=y, pos=pos, mean=mean, rstd=rstd)
    f1, f2 = fwd(), fwd()
    same("embed fwd", f1, f2)
    for k, n in (("y", rows * C), ("mean", rows), ("rstd", rows)):
        assert_written(f"embed {k}", f1[k], n)
    r = ec.embed_fwd_ref(ids, word, pos_tab, type_tab, gamma, beta, pad, eps)
    assert torch.equal(f1["pos"][:rows].long(), r["pos"].reshape(-1)), "pos_out differs from create_position_ids_from_input_ids"
    assert bool((f1["pos"][rows:] == -7).all())
    A = r["Arow"].reshape(-1)
    rs64 = r["rstd"].reshape(-1)
    check(f"embed mean C{C}", f1["mean"][:rows], r["mean"].reshape(-1), torch.zeros_like(A), {"EMB": A})
    check(f"embed rstd C{C}", f1["rstd"][:rows], rs64, torch.zeros_like(A), {"EMB": rs64 * (1 + A * rs64)})
    ik = ec.inv_keep(p) if p > 0 else 1.0
    yref = r["y"].reshape(rows, C)
    xh = ((r["x"] - r["mean"][..., None]) * r["rstd"][..., None]).reshape(rows, C)
    if p > 0:
        m = ec.mask_t(seed, rows * C, p, DEV).view(rows, C)
        yref = torch.where(m, yref * ik, torch.zeros_like(yref))
        got_kept = f1["y"][:rows * C].view(rows, C) != 0
        assert torch.equal(got_kept | (yref == 0), m | (yref == 0)), "embedding dropout mask differs from the restatement"
    gd = gamma.double().abs()[None]
    term = ik * (gd * rs64[:, None] * A[:, None] * (1 + xh.abs()) + gd * xh.abs() + beta.double().abs()[None])
    check(f"embed y C{C} p{p}", f1["y"][:rows * C].view(rows, C), yref, ec.BF16_STORE * yref.abs(), {"EMB": term})

    # backward: the table rows of absent ids / positions are the caller's zeros, dgamma / dbeta are overwritten; guards after each
    dy = rnd(rows * C, 21, 1.0).view(rows, C)
    tabs = dict(dword=(Vw, C), dpos=(S + 2, C), dtype=(2, C), dgamma=(1, C), dbeta=(1, C))
    nws = lib.load().fiber_roberta_embed_bwd_workspace(B, S, C)

    def bwd():
        out = {}
        for k, (n, c) in tabs.items():
            t = nan_buf(n * c, torch.float32)
            if k not in ("dgamma", "dbeta"):
                t[:n * c] = 0
            out[k] = t
        ws = nan_buf(nws, torch.float32)
        assert rc(lib, "fiber_roberta_embed_bwd", P(lib, dy), P(lib, ids), P(lib, f1["pos"]), P(lib, word), P(lib, pos_tab), P(lib, type_tab),
                  P(lib, gamma), P(lib, f1["mean"]), P(lib, f1["rstd"]), P(lib, out["dword"]), P(lib, out["dpos"]), P(lib, out["dtype"]),
                  P(lib, out["dgamma"]), P(lib, out["dbeta"]), P(lib, ws), B, S, C, pad, p, seed, None) == 0
        torch.cuda.synchronize()
        for k, (n, c) in tabs.items():
            assert not bool((~isnan_bits(out[k][n * c:])).any()), f"embed bwd {k}: guard written"
        assert not bool((~isnan_bits(ws[nws:])).any()), "embed bwd: written past the workspace"
        return out
    out = bwd()
    same("embed bwd", out, bwd())                              # all five tables: the same bits on every run
    assert_written("embed dgamma", out["dgamma"], C)
    assert_written("embed dbeta", out["dbeta"], C)
    dy_eff = dy.double()
    if p > 0:
        dy_eff = torch.where(m, dy_eff * ik, torch.zeros_like(dy_eff))
    ref = ec.embed_bwd_ref(ids, r["pos"], dy_eff.view(B, S, C), gamma, r["x"], f1["mean"][:rows].view(B, S), f1["rstd"][:rows].view(B, S),
                           Vw, S + 2, pad)
    for k in ("dword", "dpos"):
        rr, tt = ref[k]
        check(f"embed {k} C{C}", out[k][:rr.numel()].view(rr.shape), rr, torch.zeros_like(rr), {"EMB": tt})
        assert bool((out[k][:rr.numel()].view(rr.shape)[pad] == 0).all()), f"{k}: the pad row received a gradient"
    rr, tt = ref["dtype"]
    check(f"embed dtype C{C}", out["dtype"][:C], rr, torch.zeros_like(rr), {"EMB": tt})
    assert bool((out["dtype"][C:2 * C] == 0).all()), "dtype row 1 must stay zero"
    for k in ("dgamma", "dbeta"):
        rr, tt = ref[k]
        check(f"embed {k} C{C}", out[k][:C], rr, torch.zeros_like(rr), {"EMB": tt})


# ---- im2col ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(2, 8, 12), (3, 384, 384), (1, 4, 4)])
def test_im2col(lib, B, H, W):
    g = torch.Generator(device=DEV).manual_seed(H + W)
    img = torch.randn(B, 3, H, W, device=DEV, generator=g) * 3
    alt = torch.randn(B, 3, H, W, device=DEV, generator=g)
    rows = B * (H // 4) * (W // 4)
    cols = nan_buf(rows * 64, BF)
    assert rc(lib, "fiber_im2col_patch4", P(lib, img), P(lib, cols), B, H, W) == 0
    assert_written("im2col", cols, rows * 64)
    assert torch.equal(bits(cols[:rows * 64].view(rows, 64)), bits(ec.im2col_ref(img)))
    sel = (torch.arange(B, device=DEV) % 2 == 0).to(torch.uint8)
    cols2 = nan_buf(2 * rows * 64, BF)
    assert rc(lib, "fiber_im2col_patch4_pair", P(lib, img), P(lib, alt), P(lib, sel), P(lib, cols2), B, H, W) == 0
    assert_written("im2col pair", cols2, 2 * rows * 64)
    want = torch.cat([img, torch.where(sel.bool().view(-1, 1, 1, 1), img, alt)], 0)
    assert torch.equal(bits(cols2[:2 * rows * 64].view(2 * rows, 64)), bits(ec.im2col_ref(want)))


# ---- ABI answers ----------------------------------------------------------------------------------------------------------------------
def test_ew_abi_refusals(lib):
    """FIBER_EINVAL for every malformed call, misaligned base pointers included (checked on the host: nothing is launched);
    FIBER_OK without a launch for every zero-size call."""
    x = torch.zeros(1 << 16, dtype=BF, device=DEV)
    f = torch.zeros(1 << 16, device=DEV)
    lab = torch.zeros(64, dtype=torch.int64, device=DEV)
    b1 = x[1:].data_ptr()                                      # 2 bytes past a 16-byte boundary
    f1 = f[1:].data_ptr()
    p = lambda t: t.data_ptr()
    E = {
        "n & 7": ("fiber_gelu_bwd_bf16", p(x), p(x), p(x), 12),
        "gelu misaligned": ("fiber_gelu_bwd_bf16", b1, p(x), p(x), 16),
        "scale_add misaligned": ("fiber_scale_add_bf16", p(x), p(x), None, 1.0, b1, 16),
        "dot n & 7": ("fiber_dot_bf16", p(x), p(x), p(f), p(f), 4),
        "dot misaligned": ("fiber_dot_bf16", b1, p(x), p(f), p(f), 16),
        "dot no workspace": ("fiber_dot_bf16", p(x), p(x), p(f), None, 8 * 4096),
        "colsum N & 7": ("fiber_colsum_bf16", p(x), p(f), p(f), 4, 12, 16),
        "colsum ld & 7": ("fiber_colsum_bf16", p(x), p(f), p(f), 4, 16, 20),
        "colsum misaligned": ("fiber_colsum_bf16", b1, p(f), p(f), 4, 16, 16),
        "colsum no workspace": ("fiber_colsum_bf16", p(x), p(f), None, 4096, 8, 8),
        "gelu_colsum no workspace": ("fiber_gelu_bwd_colsum_bf16", p(x), p(x), p(x), p(f), None, 4096, 8),
        "rowscale_colsum rps 0": ("fiber_rowscale_colsum_bf16", p(x), p(f), p(x), p(f), p(f), 8, 8, 0),
        "rowscale_colsum misaligned": ("fiber_rowscale_colsum_bf16", p(x), p(f), b1, p(f), p(f), 8, 8, 1),
        "dropout p = 1": ("fiber_dropout_bf16", p(x), p(x), 16, 1.0, 0, None),
        "dropout p < 0": ("fiber_dropout_bf16", p(x), p(x), 16, -0.1, 0, None),
        "dropout misaligned": ("fiber_dropout_bf16", p(x), b1, 16, 0.1, 0, None),
        "droppath keep 0": ("fiber_droppath_scale_f32", p(f), 4, 0.0, 0, None),
        "droppath keep > 1": ("fiber_droppath_scale_f32", p(f), 4, 1.5, 0, None),
        "rowscale_add per & 7": ("fiber_rowscale_add_bf16", None, p(x), p(f), p(x), 16, 4),
        "rowscale_add misaligned": ("fiber_rowscale_add_bf16", b1, p(x), p(f), p(x), 16, 8),
        "stream_add per & 7": ("fiber_stream_add", None, 0, p(x), None, None, p(f), 12, 0.0, 0, 0.0, 0, None, None, p(x), 16),
        "stream_add res_kind": ("fiber_stream_add", p(x), 3, p(x), None, None, None, 0, 0.0, 0, 0.0, 0, None, None, p(x), 16),
        "stream_add no a": ("fiber_stream_add", None, 0, None, None, None, None, 0, 0.0, 0, 0.0, 0, None, None, p(x), 16),
        "stream_add no out": ("fiber_stream_add", None, 0, p(x), None, None, None, 0, 0.0, 0, 0.0, 0, None, None, None, 16),
        "stream_add p_b without b": ("fiber_stream_add", None, 0, p(x), None, None, None, 0, 0.0, 0, 0.1, 0, None, None, p(x), 16),
        "stream_add misaligned out32": ("fiber_stream_add", None, 0, p(x), None, None, None, 0, 0.0, 0, 0.0, 0, None, f1, None, 16),
        "stream_add misaligned res": ("fiber_stream_add", f1, 2, p(x), None, None, None, 0, 0.0, 0, 0.0, 0, None, None, p(x), 16),
        "bwd dalpha without b": ("fiber_stream_add_bwd", p(x), None, p(f), None, 0, 0.0, 0, 0.0, 0, None, None, p(x), p(f), p(f), 16),
        "bwd dalpha without db": ("fiber_stream_add_bwd", p(x), p(x), p(f), None, 0, 0.0, 0, 0.0, 0, None, None, None, p(f), p(f), 16),
        "bwd dalpha no workspace": ("fiber_stream_add_bwd", p(x), p(x), p(f), None, 0, 0.0, 0, 0.0, 0, None, None, p(x), p(f), None, 8 * 4096),
        "bwd misaligned": ("fiber_stream_add_bwd", b1, p(x), p(f), None, 0, 0.0, 0, 0.0, 0, None, None, p(x), None, None, 16),
        "cast misaligned": ("fiber_cast_f32_bf16", f1, p(x), 16),
        "ce V <= 16": ("fiber_ce_fwd_bf16", p(x), p(lab), p(f), p(f), None, 4, 16, -100),
        "ce misaligned": ("fiber_ce_fwd_bf16", b1, p(lab), p(f), p(f), None, 4, 17, -100),
        "ce bwd misaligned": ("fiber_ce_bwd_bf16", p(x), p(lab), p(f), p(f), b1, 4, 17, -100),
        "labelled no workspace": ("fiber_colsum_labelled_bf16", p(x), p(lab), p(f), None, 600, 8, -100),
        "embed C & 3": ("fiber_roberta_embed_fwd", p(lab), p(f), p(f), p(f), p(f), p(f), p(x), p(f), p(f), p(f), 1, 4, 6, 1, 1e-5, 0.0, 0, None),
        "embed C > 2048": ("fiber_roberta_embed_fwd", p(lab), p(f), p(f), p(f), p(f), p(f), p(x), p(f), p(f), p(f), 1, 4, 2052, 1, 1e-5, 0.0, 0, None),
        "embed S > 1024": ("fiber_roberta_embed_fwd", p(lab), p(f), p(f), p(f), p(f), p(f), p(x), p(f), p(f), p(f), 1, 1025, 8, 1, 1e-5, 0.0, 0, None),
        "embed misaligned table": ("fiber_roberta_embed_fwd", p(lab), f1, p(f), p(f), p(f), p(f), p(x), p(f), p(f), p(f), 1, 4, 8, 1, 1e-5, 0.0, 0, None),
        "embed misaligned y": ("fiber_roberta_embed_fwd", p(lab), p(f), p(f), p(f), p(f), p(f), b1, p(f), p(f), p(f), 1, 4, 8, 1, 1e-5, 0.0, 0, None),
        "embed bwd C & 3": ("fiber_roberta_embed_bwd", p(x), p(lab), p(f), p(f), p(f), p(f), p(f), p(f), p(f), p(f), p(f), p(f), p(f), p(f), p(f), 1, 4, 6, 1, 0.0, 0, None),
        "embed bwd misaligned dy": ("fiber_roberta_embed_bwd", b1, p(lab), p(f), p(f), p(f), p(f), p(f), p(f), p(f), p(f), p(f), p(f), p(f), p(f), p(f), 1, 4, 8, 1, 0.0, 0, None),
        "embed bwd no workspace": ("fiber_roberta_embed_bwd", p(x), p(lab), p(f), p(f), p(f), p(f), p(f), p(f), p(f), p(f), p(f), p(f), p(f), p(f), None, 1, 4, 8, 1, 0.0, 0, None),
        "embed bwd misaligned table": ("fiber_roberta_embed_bwd", p(x), p(lab), p(f), p(f), p(f), p(f), p(f), p(f), p(f), f1, p(f), p(f), p(f), p(f), p(f), 1, 4, 8, 1, 0.0, 0, None),
        "im2col H & 3": ("fiber_im2col_patch4", p(f), p(x), 1, 6, 8),
        "im2col misaligned": ("fiber_im2col_patch4", f1, p(x), 1, 4, 8),
        "im2col pair W & 3": ("fiber_im2col_patch4_pair", p(f), p(f), p(x), p(x), 1, 8, 6),
        "im2col pair misaligned cols": ("fiber_im2col_patch4_pair", p(f), p(f), p(x), b1, 1, 8, 8),
    }
    wrong = {k: v for k, (fn, *a) in E.items() if (v := rc(lib, fn, *a)) != 1}
    assert not wrong, wrong
    torch.cuda.synchronize()
    bufs = [nan_buf(256, BF), nan_buf(256, torch.float32)]
    y, o = (t.data_ptr() for t in bufs)
    OK = {
        "gelu": ("fiber_gelu_bwd_bf16", p(x), p(x), y, 0), "scale_add": ("fiber_scale_add_bf16", p(x), p(x), None, 1.0, y, 0),
        "dot": ("fiber_dot_bf16", p(x), p(x), o, None, 0), "colsum": ("fiber_colsum_bf16", p(x), o, None, 0, 8, 8),
        "colsum N 0": ("fiber_colsum_bf16", p(x), o, None, 8, 0, 8),
        "gelu_colsum": ("fiber_gelu_bwd_colsum_bf16", p(x), p(x), y, o, None, 0, 8),
        "rowscale_colsum": ("fiber_rowscale_colsum_bf16", p(x), p(f), y, o, None, 0, 8, 1),
        "fold": ("fiber_fold_rows_f32", p(f), o, 0, 8), "dropout": ("fiber_dropout_bf16", p(x), y, 0, 0.1, 0, None),
        "droppath": ("fiber_droppath_scale_f32", o, 0, 0.9, 0, None), "rowscale_add": ("fiber_rowscale_add_bf16", None, p(x), p(f), y, 0, 8),
        "stream_add": ("fiber_stream_add", None, 0, p(x), None, None, None, 0, 0.0, 0, 0.0, 0, None, None, y, 0),
        "stream_add_bwd": ("fiber_stream_add_bwd", p(x), p(x), p(f), None, 0, 0.0, 0, 0.0, 0, None, None, y, o, None, 0),
        "cast": ("fiber_cast_f32_bf16", p(f), y, 0),
        "ce fwd": ("fiber_ce_fwd_bf16", p(x), p(lab), o, o, None, 0, 100, -100),
        "ce bwd": ("fiber_ce_bwd_bf16", p(x), p(lab), p(f), p(f), y, 0, 100, -100),
        "labelled rows 0": ("fiber_colsum_labelled_bf16", p(x), p(lab), o, None, 0, 8, -100),
        "embed fwd": ("fiber_roberta_embed_fwd", p(lab), p(f), p(f), p(f), p(f), p(f), y, o, o, o, 0, 4, 8, 1, 1e-5, 0.0, 0, None),
        "embed bwd": ("fiber_roberta_embed_bwd", p(x), p(lab), p(f), p(f), p(f), p(f), p(f), p(f), p(f), o, o, o, o, o, o, 0, 4, 8, 1, 0.0, 0, None),
        "im2col B 0": ("fiber_im2col_patch4", p(f), y, 0, 8, 8),
        "im2col pair B 0": ("fiber_im2col_patch4_pair", p(f), p(f), p(x), y, 0, 8, 8),
    }
    wrong = {k: v for k, (fn, *a) in OK.items() if (v := rc(lib, fn, *a)) != 0}
    assert not wrong, wrong
    torch.cuda.synchronize()
    for i, t in enumerate(bufs):
        assert bool(isnan_bits(t).all()), f"buffer {i} written by a zero-size call"


def test_wrappers_copy_misaligned_views(lib):
    """ops wrappers given contiguous views at an odd element offset copy them (the ABI refuses such a base) and compute what they
    compute on an aligned copy"""
    from fiber_amd import ops
    n = 8 * 999
    big = rnd(n + 1, 30)
    a = big[1:]
    assert a.is_contiguous() and a.data_ptr() % 16
    res = rnd(n, 31)
    y1 = ops.stream_add(res, a)
    y2 = ops.stream_add(res, a.clone())
    assert torch.equal(y1.view(torch.int16), y2.view(torch.int16))
    V = 1001
    lg = rnd(4 * V + 3, 32, 3.0)[3:].view(4, V)
    lab = torch.tensor([0, 5, -100, V - 1], device=DEV)
    l1 = ops.cross_entropy(lg, lab)
    l2 = ops.cross_entropy(lg.clone(), lab)
    assert torch.equal(l1, l2)
    assert torch.equal(ops.colsum(rnd(8 * 64 + 1, 33)[1:].view(64, 8)), ops.colsum(rnd(8 * 64 + 1, 33)[1:].view(64, 8).clone()))


# ---- launched kernels -------------------------------------------------------------------------------------------------------------------
PROBE_EXPECTED = {
    "stream_add res0": ["stream_add_kernel<0>"], "stream_add res1": ["stream_add_kernel<1>"], "stream_add res2": ["stream_add_kernel<2>"],
    "stream_add_bwd dalpha 1 block": ["stream_add_bwd_kernel"], "stream_add_bwd dalpha": ["colsum_fold_kernel", "stream_add_bwd_kernel"],
    "dot 1 block": ["dot_kernel"], "dot": ["colsum_fold_kernel", "dot_kernel"],
    "colsum": ["colsum_kernel"], "colsum slabs": ["colsum_fold_kernel", "colsum_kernel"],
    "gelu_bwd_colsum": ["gelu_bwd_colsum_kernel"], "gelu_bwd_colsum slabs": ["colsum_fold_kernel", "gelu_bwd_colsum_kernel"],
    "rowscale_colsum": ["rowscale_colsum_kernel"], "rowscale_colsum slabs": ["colsum_fold_kernel", "rowscale_colsum_kernel"],
    "colsum_labelled": ["colsum_labelled_kernel"], "colsum_labelled slabs": ["colsum_fold_kernel", "colsum_labelled_kernel"],
    "im2col": ["im2col4_kernel<false>"], "im2col pair": ["im2col4_kernel<true>"],
    **{f"embed fwd C{c}": [f"roberta_embed_fwd_kernel<{nv}>"] for c, nv in ((256, 1), (512, 2), (1024, 4), (2048, 8))},
    **{f"embed bwd C{c}": ["embed_rank_kernel", "embed_segsum_kernel", f"roberta_embed_bwd_kernel<{nv}>"]
       for c, nv in ((256, 1), (512, 2), (1024, 4), (2048, 8))},
}


def test_ew_paths_probe_names_the_declared_kernels():
    """tools/probes/ew_paths.py runs each entry point once per path under torch.profiler in a child process: each call launched exactly
    the kernels it declares -- every stream_add / embedding / im2col template, each column sum with and without its fold."""
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = run_bounded([sys.executable, os.path.join(ROOT, "tools", "probes", "ew_paths.py")], 300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    seen = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert seen == PROBE_EXPECTED, {k: (seen.get(k), v) for k, v in PROBE_EXPECTED.items() if seen.get(k) != v}
