"""Case table of the optimizer kernels (csrc/optim.hip): fiber_adamw_multi_f32 with hand-built tables, fiber_transpose_multi_bf16 and
fiber_rowperm_cast_multi_bf16 with hand-built descriptors; the fp64 reference of one AdamW step and its per-element bounds.  Shared by
tests/test_hip_optim_paths.py, tests/test_dcn_optim_compare_host.py and tools/probes/dcn_optim_paths.py.  Importing it needs no GPU.

One step, from the fp32 state and the fp32 hyper-parameters as the kernel receives them (adam1 in optim.hip), in fp64:
  m' = b1 m + (1 - b1) g            v' = b2 v + (1 - b2) g g            (1 - b1, 1 - b2 formed in fp32)
  p1 = p - step_size m' / (sqrt(v') + eps)            p' = p1 - (lr wd) p1
  step_size = float32(double(lr) sqrt(1 - b2^t) / (1 - b1^t)), or hyper[1] (and lr = hyper[0]) when the device words are given.
Bounds, |got - ref| <= CONST[c] 2^-24 term + 2^-147 (fp32 denormal results: 2^-150 an operation); the compiler may contract to FMA:
  M   term = |b1 m| + |(1 - b1) g|                2 products, 1 sum                          ceiling 2 x 3
  V   term = |b2 v| + |(1 - b2) g g|              3 products, 1 sum                          ceiling 2 x 4
  P   term = |p| + |update| + |decay|, the reference taken from the m', v' the kernel STORED (what it divides by): sqrt, + eps, /, * step_size,
      p - update, lr wd, * p1, p1 - decay                                                     ceiling 2 x 8
The bf16 working copy equals bf16(p') of the stored p' to the bit."""
import math

import numpy as np
import torch

F32 = 2.0 ** -24
TINY32 = 2.0 ** -147
CONST = {"M": 2.0, "V": 2.0, "P": 4.0}     # MI355X needed: see profiles/dcn_optim_pins.md
CEILING = {"M": 6.0, "V": 8.0, "P": 16.0}
CHUNK = 4096
GUARD = 16
SENTINEL = -7.25                            # guard value of p, m, v and the bf16 copy (bf16-exact)

# (numel, gradient bytes past 16-byte alignment, p / m / v bytes into their allocation, bf16 copy: None | bytes into its allocation)
TENSORS = [
    (1, 0, 0, 0), (3, 4, 0, None), (4, 8, 0, 0), (5, 12, 0, 0), (4095, 0, 0, 0),
    (4096, 4, 0, 0),                        # a full chunk with a misaligned gradient
    (4097, 0, 0, None), (8192 + 7, 8, 0, 0), (3 * 4096, 0, 0, 0),
    (4096 + 5, 0, 4, 0),                    # p, m, v views 4 bytes into an allocation: the scalar path
    (4096 + 3, 0, 0, 2),                    # the bf16 copy 2 bytes into an allocation: also scalar
    (4096, 12, 0, None),
]
ADAM_CASES = [
    dict(name="step1", step=1, lr=1e-4, wd=0.01, b1=0.9, b2=0.98, eps=1e-8, hyper=False),
    dict(name="step1000_wd0", step=1000, lr=3e-5, wd=0.0, b1=0.9, b2=0.98, eps=1e-8, hyper=False),
    dict(name="hyper", step=1000, lr=3e-5, wd=0.01, b1=0.9, b2=0.98, eps=1e-8, hyper=True),   # by value: lr x 7 and step 3, both wrong
]
ADAM_BY_NAME = {c["name"]: c for c in ADAM_CASES}


def chunk_table():
    """(tensor, chunk) pairs: tensors in reverse order, the chunks of tensors 7 and 8 interleaved"""
    per = {i: [(i, c) for c in range(-(-n // CHUNK))] for i, (n, *_r) in enumerate(TENSORS)}
    inter = [p for pair in zip(per[7], per[8]) for p in pair]
    rest = [p for i in reversed(range(len(TENSORS))) if i not in (7, 8) for p in per[i]]
    return rest[:5] + inter + rest[5:]


def step_size(case):
    lr, b1, b2 = (float(np.float32(case[k])) for k in ("lr", "b1", "b2"))
    return np.float32(lr * math.sqrt(1.0 - b2 ** case["step"]) / (1.0 - b1 ** case["step"]))


def make_state(case, seed=0):
    """per tensor: p, g, m, v float32 numpy.  Gradients hold 0 (with m = v = 0), 1e-20 and 1e15 where the tensor is long enough."""
    g_ = torch.Generator().manual_seed(77 + seed)
    out = []
    for n, *_r in TENSORS:
        p = torch.randn(n, generator=g_).numpy()
        g = (torch.randn(n, generator=g_) * 0.02).numpy()
        m = (torch.randn(n, generator=g_) * 0.01).numpy()
        v = (torch.randn(n, generator=g_) * 0.01).numpy() ** 2
        if n >= 5:
            g[1], m[1], v[1] = 0.0, 0.0, 0.0
            g[2], g[n - 1] = 1e-20, 1e15
            g[3], m[3], v[3] = 1e-20, 0.0, 0.0
        out.append(dict(p=p.astype(np.float32), g=g.astype(np.float32), m=m.astype(np.float32), v=v.astype(np.float32)))
    return out


def hyper_scalars(case):
    """(lr, wd, b1, b2, eps, step_size) as the fp32 values the kernel computes with"""
    f = lambda k: np.float32(case[k])
    return f("lr"), f("wd"), f("b1"), f("b2"), f("eps"), step_size(case)


def moments_reference(case, st):
    """-> m', v' (fp64) and their bound terms"""
    lr, wd, b1, b2, eps, ss = hyper_scalars(case)
    omb1, omb2 = float(np.float32(1) - b1), float(np.float32(1) - b2)
    g, m, v = (st[k].astype(np.float64) for k in ("g", "m", "v"))
    m1, v1 = float(b1) * m + omb1 * g, float(b2) * v + omb2 * g * g
    return m1, v1, np.abs(float(b1) * m) + np.abs(omb1 * g), np.abs(float(b2) * v) + np.abs(omb2 * g * g)


def param_reference(case, p, m1, v1):
    """p' (fp64) from the moments given (the kernel's stored ones on the GPU, the reference's on the host) and its bound term"""
    lr, wd, b1, b2, eps, ss = hyper_scalars(case)
    upd = float(ss) * (m1 / (np.sqrt(v1) + float(eps)))
    p1 = p.astype(np.float64) - upd
    decay = float(lr) * float(wd) * p1
    return p1 - decay, np.abs(p.astype(np.float64)) + np.abs(upd) + np.abs(decay)


def bf16_bits(a):
    """round-to-nearest-even bf16 bit patterns (uint16) of a float32 array, by integer arithmetic; infinities and denormals included"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


# ---- transpose / row-permuted cast ---------------------------------------------------------------------------------------------------------
SHAPES = [(8, 8), (64, 64), (72, 136), (200, 8), (8, 200)]
DESC_SETS = {"one": [2], "two": [3, 0], "five": [0, 1, 2, 3, 4]}        # indices into SHAPES, in table order
PERM_SETS = {"one": [(2, True, True)], "two": [(0, True, True), (3, False, True)],
             "five": [(0, True, False), (1, True, True), (2, False, True), (3, True, True), (4, True, False)]}   # (shape, dst_t, bias)


def probe_cases():
    """name -> the kernel the case launches, for tools/probes/dcn_optim_paths.py"""
    d = {f"adam:{c['name']}": ["adamw_multi_kernel"] for c in ADAM_CASES}
    d.update({f"transpose:{k}": ["transpose_multi_kernel"] for k in DESC_SETS})
    d.update({f"rowperm:{k}": ["rowperm_cast_multi_kernel"] for k in PERM_SETS})
    return d


def tiles_of(N, K):
    return -(-N // 64) * -(-K // 64), -(-K // 64)


def perm_of(N):
    """a non-identity permutation: blocks of 8 reversed, then rotated by 3"""
    p = np.arange(N).reshape(-1, 8)[:, ::-1].reshape(-1)
    return np.roll(p, 3).astype(np.int32)


def special_f32(N, K, seed):
    """fp32 sources: normal values, bf16 round-to-even ties in both directions, -0.0, +-inf and fp32 denormals"""
    g_ = torch.Generator().manual_seed(300 + seed)
    a = torch.randn(N, K, generator=g_).numpy().astype(np.float32).reshape(-1)
    sp = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -0.0, np.inf, -np.inf, 2.0 ** -130, -3 * 2.0 ** -149, 2.0 ** -134,
                   3 * 2.0 ** -134, 1 + 2.0 ** -8 + 2.0 ** -20], np.float32)
    for i, s in enumerate(sp):
        a[(7 * i + 3) % a.size::97][:3] = s
    return a.reshape(N, K)


# ---- runners -------------------------------------------------------------------------------------------------------------------------------
def _view(n, byte_off, dtype, fill, device):
    """an n-element view `byte_off` bytes into a fresh allocation, SENTINEL in front of it and in the GUARD elements after it"""
    sz = torch.empty(0, dtype=dtype).element_size()
    lead = byte_off // sz
    buf = torch.full((lead + n + GUARD,), SENTINEL, dtype=dtype, device=device)
    if fill is not None:
        buf[lead:lead + n] = fill
    return buf, buf[lead:lead + n]


def run_adam(lib, case, state, device="cuda"):
    """One launch over TENSORS.  -> per tensor the buffers (with guards) and views of p, m, v, w after the step."""
    bufs = []
    for (n, goff, poff, woff), st in zip(TENSORS, state):
        d = {}
        for k in ("p", "m", "v"):
            d[k + "_buf"], d[k] = _view(n, poff, torch.float32, torch.from_numpy(st[k]).to(device), device)
        d["g_buf"], d["g"] = _view(n, goff, torch.float32, torch.from_numpy(st["g"]).to(device), device)
        if woff is not None:
            d["w_buf"], d["w"] = _view(n, woff, torch.bfloat16, None, device)
        assert d["g"].data_ptr() % 16 == goff and d["p"].data_ptr() % 16 == poff
        bufs.append(d)
    table = torch.tensor([[d["p"].data_ptr(), d["g"].data_ptr(), d["m"].data_ptr(), d["v"].data_ptr(), d["w"].data_ptr() if "w" in d else 0]
                          for d in bufs], dtype=torch.int64).to(device)
    numel = torch.tensor([t[0] for t in TENSORS], dtype=torch.int64).to(device)
    chunks = torch.tensor(chunk_table(), dtype=torch.int32).to(device)
    lr, wd, b1, b2, eps, ss = hyper_scalars(case)
    hyper, lr_arg, step_arg = None, float(lr), case["step"]
    if case["hyper"]:
        hyper = torch.tensor([float(lr), float(ss)], dtype=torch.float32).to(device)
        lr_arg, step_arg = float(lr) * 7, 3
    lib.call("fiber_adamw_multi_f32", lib.ptr(table), lib.ptr(numel), lib.ptr(chunks), chunks.shape[0], lr_arg, float(wd), float(b1), float(b2),
             float(eps), step_arg, lib.ptr(hyper))
    torch.cuda.synchronize()
    return bufs


def _nan16(n, device):
    return torch.full((n,), -32768 + 0x7FC0, dtype=torch.int16, device=device).view(torch.bfloat16)


def run_transpose(lib, which, device="cuda"):
    """-> [(src, dst buffer with GUARD, N, K)] after ONE launch over the descriptors of DESC_SETS[which]"""
    g_ = torch.Generator().manual_seed(5)
    recs, rows, tile0 = [], [], 0
    for i in DESC_SETS[which]:
        N, K = SHAPES[i]
        src = torch.randint(-32768, 32767, (N, K), generator=g_, dtype=torch.int16).to(device).view(torch.bfloat16)
        dst = _nan16(N * K + GUARD, device)
        nt, tk = tiles_of(N, K)
        rows.append([src.data_ptr(), dst.data_ptr(), N | (K << 32), tile0 | (tk << 32)])
        recs.append((src, dst, N, K))
        tile0 += nt
    table = torch.tensor(rows, dtype=torch.int64).to(device)
    lib.call("fiber_transpose_multi_bf16", lib.ptr(table), len(rows), tile0)
    torch.cuda.synchronize()
    return recs


def run_rowperm(lib, which, device="cuda"):
    """-> [dict(src, perm, bias, dst, dst_t, bias_dst, N, K)] (numpy sources, device destinations with GUARD) after ONE launch"""
    recs, rows, tile0, keep = [], [], 0, []
    for j, (i, with_t, with_bias) in enumerate(PERM_SETS[which]):
        N, K = SHAPES[i]
        src, perm = special_f32(N, K, j), perm_of(N)
        bias = special_f32(1, N, 50 + j).reshape(-1) if with_bias else None
        d = dict(src=src, perm=perm, bias=bias, N=N, K=K, dst=_nan16(N * K + GUARD, device),
                 dst_t=_nan16(N * K + GUARD, device) if with_t else None,
                 bias_dst=torch.full((N + GUARD,), -4194304, dtype=torch.int32, device=device).view(torch.float32))
        dev = [torch.from_numpy(src).to(device), torch.from_numpy(perm).to(device), None if bias is None else torch.from_numpy(bias).to(device)]
        keep.append(dev)
        nt, tk = tiles_of(N, K)
        rows.append([dev[0].data_ptr(), dev[1].data_ptr(), d["dst"].data_ptr(), d["dst_t"].data_ptr() if with_t else 0,
                     dev[2].data_ptr() if with_bias else 0, d["bias_dst"].data_ptr(), N | (K << 32), tile0 | (tk << 32)])
        recs.append(d)
        tile0 += nt
    table = torch.tensor(rows, dtype=torch.int64).to(device)
    lib.call("fiber_rowperm_cast_multi_bf16", lib.ptr(table), len(rows), tile0)
    torch.cuda.synchronize()
    return recs
