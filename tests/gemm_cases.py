"""Case table of the NT GEMM path matrix: every (kernel template, epilogue) pair that fiber_gemm_nt_bf16 reaches with the default
environment, at a shape that sends the call to that template.  Shared by tests/test_hip_gemm_paths.py (values against fp64) and
tools/probes/gemm_paths.py (which kernel each case actually launched).

Kernels (gemm.hip) and the shapes that select them:
  q8      gemm_nt_q8_kernel              >= 200 256x256 tiles, N % 256 == 0          (persistent, wave-private epilogue)
  q8p     gemm_nt_q8_kernel              the same with a partial last tile column (N % 64 == 0, N > 256)
  persist gemm_nt_wide_persist_kernel    the wide shape for the epilogues q8 is not built for (GELU + residual, fp32 stream without
                                         a row scale)
  r256    gemm_nt_glds_kernel<256, 128>  >= 400 256x128 tiles and K >= 256, not a wide shape
  r128    gemm_nt_glds_kernel<128, 128>  >= 192 128x128 tiles
  r64     gemm_nt_glds_kernel<64, 64>    fewer tiles
  reg128  gemm_nt_kernel<128, 128>       K % 64 != 0 or N % 8 != 0 (no LDS-DMA), >= 192 tiles; fp32 outputs
  reg64   gemm_nt_kernel<64, 64>         the same, fewer tiles
These are all the NT GEMM kernels gemm.hip builds (the trace form of q8 apart: tools/gemm_trace.py).
Every case has a ragged last row tile, a ragged last column tile where the kernel allows one, and a row-strided X (ldx > K)."""
import torch

# kernel -> (M, N, K, ldx): ragged M / N where allowed, X rows padded
SHAPES = {
    "q8": (25729, 512, 192, 232), "q8p": (16513, 832, 128, 136), "persist": (25729, 512, 256, 296),
    "r256": (25729, 392, 256, 264), "r128": (6273, 392, 320, 360), "r64": (1000, 200, 192, 200),
    "reg128": (6273, 396, 72, 80), "reg64": (1000, 196, 72, 88),
}
# epilogue -> ops.gemm_nt features: b bias, r bf16 residual, s row scale, g GELU, p pre-activation copy, d gelu' * aux,
# c column sums, t fp32 residual stream (+ bf16 shadow), f fp32 output
EPILOGUES = {
    "plain": "", "bias": "b", "rs": "s", "res": "br", "res_rs": "brs", "gelu": "bg", "gelu_pre": "bgp", "gelu_pre_rs": "bgps",
    "gelu_res": "bgpr", "gelu_res_rs": "bgprs", "ggrad": "d", "ggrad_rs": "ds", "ggrad_colsum": "dc", "ggrad_colsum_rs": "dcs",
    "s32": "bt", "s32_rs": "bts", "f32": "bf",
}
_Q8 = ["plain", "bias", "rs", "res", "res_rs", "gelu", "gelu_pre", "gelu_pre_rs", "ggrad", "ggrad_rs", "s32_rs"]
_RING = ["plain", "bias", "rs", "res", "res_rs", "gelu", "gelu_pre", "gelu_pre_rs", "gelu_res", "ggrad", "ggrad_rs", "ggrad_colsum",
         "ggrad_colsum_rs", "s32", "s32_rs"]
_REG = ["plain", "bias", "rs", "res", "res_rs", "gelu", "gelu_pre", "gelu_pre_rs", "gelu_res", "s32", "s32_rs", "f32"]
# (a residual without a row scale reaches q8 only with whole tile columns: on the partial-column shape it takes the 128x128 kernel)
PAIRS = {"q8": _Q8, "q8p": [e for e in _Q8 if e != "res"], "persist": ["gelu_res", "gelu_res_rs", "s32"], "r256": _RING, "r128": _RING, "r64": _RING,
         "reg128": _REG, "reg64": _REG}


def _case(name, kernel, epi, M, N, K, ldx, rps=None):
    return dict(name=name, kernel=kernel, epi=epi, M=M, N=N, K=K, ldx=ldx, rps=rps or (M // 9 + 1))


CASES = [_case(f"{k}-{e}", k, e, *SHAPES[k]) for k in PAIRS for e in PAIRS[k]]
CASES += [
    # the bench's stage-0 MLP at B = 32 (9216 tokens a sample): outputs of 302 MB - 1.2 GB take the streaming stores
    _case("stream-fc1-gelu_pre", "q8", "gelu_pre", 294912, 2048, 512, 512, 9216),
    _case("stream-fc2-res_rs", "q8", "res_rs", 294912, 512, 2048, 2048, 9216),
    _case("stream-fc1dgrad-ggrad_rs", "q8", "ggrad_rs", 294912, 2048, 512, 512, 9216),
    # gelu' * aux with column sums at K = 128: the 128x128 kernel, whose colpart has ceil(M / 128) rows (fiber_gemm_row_tile)
    _case("colsum-k128-ggrad_colsum", "r128", "ggrad_colsum", 65536, 512, 128, 128),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}

# kernel -> the template family it must reach (q8 and q8p: one template, full / partial last tile column)
FAMILIES = {"q8": "gemm_nt_q8_kernel<", "q8p": "gemm_nt_q8_kernel<", "persist": "gemm_nt_wide_persist_kernel<",
            "r256": "gemm_nt_glds_kernel<256, 128,", "r128": "gemm_nt_glds_kernel<128, 128,", "r64": "gemm_nt_glds_kernel<64, 64,",
            "reg128": "gemm_nt_kernel<128, 128>", "reg64": "gemm_nt_kernel<64, 64>"}
_RING_GEOM = {"r256": "256, 128, 4, 2, 3", "r128": "128, 128, 2, 2, 2", "r64": "64, 64, 2, 2, 2"}


def expected_kernel(case):
    """The kernel template (as the profiler spells it) the dispatcher must launch for `case`."""
    f = EPILOGUES[case["epi"]]
    k = case["kernel"]
    if k.startswith("reg"):
        return "gemm_nt_kernel<128, 128>" if k == "reg128" else "gemm_nt_kernel<64, 64>"
    epi = 1 if "g" in f else 2 if "d" in f else 3 if "t" in f else 0
    has_r = "r" in f or "t" in f
    has_rs = "s" in f or (k.startswith("q8") and f == "br")     # q8 serves the residual without a scale with a scale of 1.0
    tf = lambda v: "true" if v else "false"
    if k.startswith("q8"):
        return f"gemm_nt_q8_kernel<{epi}, {tf(has_r)}, {tf(has_rs)}, false>"
    if k == "persist":
        return f"gemm_nt_wide_persist_kernel<2, 4, {epi}, {tf(has_r)}, {tf(has_rs)}>"
    return f"gemm_nt_glds_kernel<{_RING_GEOM[k]}, {epi}, {tf(has_r)}, {tf(has_rs)}>"


def make_inputs(case, device="cuda", seed=0):
    """bf16 operands with structure a transposed / swapped operand cannot match: X has a non-zero mean and columns of unequal scale,
    W rows of unequal scale; the row scale drops sample 1 and gives every other sample its own factor."""
    M, N, K, ldx = case["M"], case["N"], case["K"], case["ldx"]
    f = EPILOGUES[case["epi"]]
    g = torch.Generator(device=device).manual_seed(seed + M + 7 * N + 31 * K)
    bf = torch.bfloat16
    xs = torch.empty(M, ldx, device=device, dtype=bf)
    xs[:, :K] = ((torch.randn(M, K, device=device, generator=g) + 0.5) * torch.linspace(0.5, 2.0, K, device=device)).to(bf)
    xs[:, K:] = float("nan")                                 # the padding of a strided X must never be read
    inp = {"x": xs[:, :K]}
    inp["w"] = (torch.randn(N, K, device=device, generator=g) * K ** -0.5 * torch.linspace(1.5, 0.5, N, device=device)[:, None]).to(bf)
    if "b" in f:
        inp["bias"] = torch.randn(N, device=device, generator=g) * 0.5
    if "r" in f:
        inp["residual"] = torch.randn(M, N, device=device, generator=g).to(bf)
    if "t" in f:
        inp["res32"] = torch.randn(M, N, device=device, generator=g) * 2.0
    if "s" in f:
        ns = -(-M // case["rps"])
        rs = 0.5 + 0.0625 * torch.arange(ns, device=device, dtype=torch.float32)
        rs[1] = 0.0
        inp["rowscale"] = rs
    if "d" in f:
        inp["aux"] = (torch.randn(M, N, device=device, generator=g) * 1.5).to(bf)
    return inp


def run(ops, case, inp):
    """One ops.gemm_nt call of `case` -> {"y", "pre", "y32", "colsum"} (the ones the epilogue produces)."""
    f = EPILOGUES[case["epi"]]
    kw = dict(bias=inp.get("bias"), residual=inp.get("residual"), rowscale=inp.get("rowscale"),
              rows_per_sample=case["rps"] if "s" in f else 0)
    if "t" in f:
        y, y32 = ops.gemm_nt(inp["x"], inp["w"], kw["bias"], None, 0, False, kw["rowscale"], kw["rows_per_sample"], res32=inp["res32"])
        return {"y": y, "y32": y32}
    if "d" in f:
        y, e = ops.gemm_nt(inp["x"], inp["w"], None, None, 2, False, kw["rowscale"], kw["rows_per_sample"], aux=inp["aux"],
                           want_colsum="c" in f)
        return {"y": y, "colsum": e} if "c" in f else {"y": y}
    y, pre = ops.gemm_nt(inp["x"], inp["w"], act=1 if "g" in f else 0, want_pre="p" in f, out_fp32="f" in f, **kw)
    return {"y": y, "pre": pre} if "p" in f else {"y": y}
