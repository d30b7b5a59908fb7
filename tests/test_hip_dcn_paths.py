"""Every deformable-convolution kernel path, element by element against fp64 (tests/dcn_cases.py: the case table, the reference, the
bounds).  Each case calls the C ABI directly with every output NaN-filled and GUARD elements after it: every owned element must be
written, no guard may change; the tiled input gradient runs with the window part of its workspace NaN-filled (the kernels must write
every word they later read), the part the contract wants zero zeroed, and guard words after it.  No element of any output is left out:
the reference forms the sampling coordinate with the same single fp32 addition, so floor, the `in` test and the corner flags agree.
dmask / doffset of two runs are bit-equal; dx of the scatter goes through fp32 atomics and is bounded instead; the tiled dx is
bit-equal whenever nothing leaves a window.  FIBER_DCN_CALIBRATE=<file> records, per constant of dcn_cases.CONST, the largest value
any element needed (the others held); every constant stays at or below the ceiling dcn_cases.ceilings() derives for the case.

Not covered: the grid cap of 262 144 workgroups in the gather and scatter launches (the grid-stride loops above it): reaching it needs
about 1 GB of columns."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import dcn_cases as dc
from tests.hip_util import BF, DEV, assert_elementwise
from tests.mp_util import run_bounded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONST = dc.CONST
_CAL = os.environ.get("FIBER_DCN_CALIBRATE")
_needed = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from fiber_amd import lib
    lib.load()
    return lib


def T64(a):
    return torch.from_numpy(np.array(a)).to(torch.float64)


def check(name, got, ref, spec):
    """assert_elementwise with bound = base + sum_c CONST[c] * terms[c] (numpy reference / terms, 2-D views)"""
    base, terms = spec
    ref = T64(ref)
    ref = ref.reshape(-1, ref.shape[-1])
    got = got.detach().cpu().to(torch.float64).reshape(ref.shape)
    base = T64(base).reshape(ref.shape)
    terms = {c: T64(t).reshape(ref.shape) for c, t in terms.items()}
    bound = base + sum(CONST[c] * t for c, t in terms.items())
    if _CAL:
        err = (got - ref).abs()
        for c, t in terms.items():
            rest = base + sum(CONST[o] * x for o, x in terms.items() if o != c)
            need = ((err - rest) / t.clamp_min(1e-300)).where(t > 0, torch.zeros_like(err)).max().item()
            if need > _needed.get(c, (0.0, ""))[0]:
                _needed[c] = (need, name)
        with open(_CAL, "w") as f:
            json.dump(_needed, f, indent=1)
    return assert_elementwise(name, got, ref, bound)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _nan(t):
    return _bits(t) == (dc.NAN_BF16 if t.dtype == torch.bfloat16 else dc.NAN_F32)


def assert_written(name, buf, n):
    """the first n elements of buf written, the rest (the guard) untouched"""
    missed = int(_nan(buf[:n]).sum())
    stray = int((~_nan(buf[n:])).sum())
    assert missed == 0, f"{name}: {missed} owned elements never written (first at {torch.nonzero(_nan(buf[:n]))[0].tolist()})"
    assert stray == 0, f"{name}: {stray} guard elements written"


def assert_same(name, a, b, keys=None):
    for k in (keys or a):
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{name}: {k} differs between two runs"


def _below_ceiling(case, ref):
    top = dc.ceilings(case, int(ref["dx_n"].max()) if "dx_n" in ref else 0)
    assert all(CONST[k] <= top[k] for k in CONST), (case["name"], CONST, top)


# ---- gather --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in dc.GATHER_CASES])
def test_gather_path(lib, name):
    case = dc.CASE_BY_NAME[name]
    inp = dc.make_inputs(case)
    dev = dc.to_device(inp)
    n = case["M"] * case["T"] * case["C"]
    o1, o2 = dc.run_gather(lib, case, dev), dc.run_gather(lib, case, dev)
    torch.cuda.synchronize()
    assert_same(name, o1, o2)
    assert_written(f"{name} cols", o1["cols"], n)
    ref = dc.reference(case, inp, grads=False)
    _below_ceiling(case, ref)
    got = o1["cols"][:n].view(case["M"], -1)
    check(f"{name} cols", got, ref["cols"], dc.bound_terms(case, ref)["cols"])
    if case["off"] is None and not case["mask"]:               # every weight is 0 or 1: the im2col of x, to the bit
        want = torch.from_numpy(dc.im2col(case, inp["x"])).to(BF)
        assert torch.equal(_bits(got.cpu()), _bits(want)), f"{name}: not the im2col of x bit for bit"
    if case["off"] == "outside":                               # nothing is taken: every column is +0
        assert int(_bits(got).ne(0).sum()) == 0, f"{name}: a column that is not +0"


# ---- scatter -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in dc.SCATTER_CASES])
def test_scatter_path(lib, name):
    case = dc.CASE_BY_NAME[name]
    inp = dc.make_inputs(case)
    dev = dc.to_device(inp)
    plain = case["off"] is None
    want = ("dx",) if plain else ("dx", "doffset", "dmask")
    o1, o2 = dc.run_scatter(lib, case, dev, want), dc.run_scatter(lib, case, dev, want)
    torch.cuda.synchronize()
    assert_same(name, o1, o2, [k for k in want if k != "dx"])
    ref = dc.reference(case, inp)
    _below_ceiling(case, ref)
    spec = dc.bound_terms(case, ref)
    sizes = dict(dx=ref["dx"].size, doffset=ref["doffset"].size, dmask=ref["dmask"].size)
    for k in want:
        assert_written(f"{name} {k}", o1[k], sizes[k])
        for o in (o1, o2):
            check(f"{name} {k}", o[k][:sizes[k]], ref[k], spec[k])


def test_scatter_null_outputs(lib):
    """every combination of dx, doffset, dmask that ops._DeformConv.backward can pass: what is asked for is what a full call gives
    (dmask, doffset to the bit; dx within its bound), nothing else is written"""
    case = dc.CASE_BY_NAME["s_c16_s1"]
    inp = dc.make_inputs(case)
    dev = dc.to_device(inp)
    ref = dc.reference(case, inp)
    spec = dc.bound_terms(case, ref)
    full = dc.run_scatter(lib, case, dev)
    for want in (("dx",), ("doffset",), ("dmask",), ("dx", "doffset"), ("dx", "dmask"), ("doffset", "dmask")):
        o = dc.run_scatter(lib, case, dev, want)
        torch.cuda.synchronize()
        for k in want:
            n = ref[k].size
            assert_written(f"{want} {k}", o[k], n)
            if k == "dx":
                check(f"{want} dx", o[k][:n], ref[k], spec[k])
            else:
                assert torch.equal(_bits(o[k]), _bits(full[k])), f"{want}: {k} differs from the full call"


# ---- tiled input gradient ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in dc.TILED_CASES])
def test_tiled_dx_path(lib, name):
    case = dc.CASE_BY_NAME[name]
    inp = dc.make_inputs(case)
    dev = dc.to_device(inp)
    o1, o2 = dc.run_tiled(lib, case, dev), dc.run_tiled(lib, case, dev)
    torch.cuda.synchronize()
    n = case["B"] * case["H"] * case["W"] * case["C"]
    assert_written(f"{name} dx", o1["dx"], n)
    words, zero = o1["words"], o1["zero"]
    ws = o1["ws"]
    assert not bool(_nan(ws[:words - zero]).any()), f"{name}: window words never written"
    assert bool(_nan(ws[words:]).all()), f"{name}: written past the workspace"
    ref = dc.reference(case, inp)
    _below_ceiling(case, ref)
    if ref["n_far"].sum() == 0:                                # nothing leaves a window: no atomics, two runs agree to the bit
        assert_same(name, o1, o2, ["dx"])
        assert int(_bits(ws[words - zero:words - 4]).ne(0).sum()) == 0, f"{name}: the far map was touched"
    got = o1["dx"][:n]
    for o in (o1, o2):
        check(f"{name} dx", o["dx"][:n], ref["dx"], dc.bound_terms(case, ref)["dx_tiled"])
    if case["dcols"] == "zero":
        assert int(_bits(got).ne(0).sum()) == 0, f"{name}: an output that is not +0"
    if case["dcols"] == "pile":                                # the int32 window accumulator (and the sum over the windows) did not wrap
        y, x = case["off"][1], case["off"][2]
        v = got.view(case["H"], case["W"], case["C"])[y, x].float().cpu()
        total = ref["dx_n"].max() * dc.PILE_VALUE
        assert bool((v - total).abs().max() <= 2.0 ** -8 * total), (v.tolist(), total)


def test_dx_workspace_formula(lib):
    for case in dc.TILED_CASES:
        got = lib.plain("fiber_dcn_dx_workspace", case["B"], case["H"], case["W"], case["C"], case["Ho"], case["Wo"], case["stride"])
        assert got == dc.workspace_words(case), case["name"]
    assert lib.plain("fiber_dcn_dx_workspace", 1, 16, 16, 24, 16, 16, 1) == -1          # C = 24: not a multiple of 16
    assert lib.plain("fiber_dcn_dx_workspace", 1, 16, 16, 16, 6, 6, 3) == -1            # stride 3


def test_dcn_abi_refusals(lib):
    """C = 12, Ho inconsistent with H, and for the tiled form a 5 x 5 kernel, pad 0, stride 3, C = 24: FIBER_EINVAL before any launch, the
    NaN-filled outputs untouched"""
    P = lib.ptr
    s = torch.cuda.current_stream().cuda_stream
    L = lib.load()
    x = torch.zeros(1 * 16 * 16 * 24, dtype=BF, device=DEV)
    dcols = torch.zeros(16 * 16 * 25 * 24, dtype=BF, device=DEV)
    outs = [dc.nan_buf(16 * 16 * 25 * 24, BF), dc.nan_buf(16 * 16 * 24, torch.float32), dc.nan_buf(16 * 16 * 50, torch.float32),
            dc.nan_buf(16 * 16 * 25, torch.float32), dc.nan_buf(16 * 16 * 24, BF), dc.nan_buf(1 << 16, torch.float32)]
    cols, dx, doff, dmask, dxb, ws = outs
    for C, H, Ho in ((12, 4, 4), (16, 4, 5)):
        assert L.fiber_dcn_gather_bf16(P(x), None, None, P(cols), 1, H, 4, C, Ho, 4, 3, 3, 1, 1, s) == 1
        assert L.fiber_dcn_scatter_bf16(P(dcols), P(x), None, None, P(dx), P(doff), P(dmask), 1, H, 4, C, Ho, 4, 3, 3, 1, 1, s) == 1
        assert L.fiber_dcn_dx_bf16(P(dcols), None, None, P(dxb), P(ws), 1, H, 4, C, Ho, 4, 3, 3, 1, 1, s) == 1
    #                          C   Ho  k  stride pad
    for C, Ho, k, st, pad in ((16, 14, 5, 1, 1), (16, 14, 3, 1, 0), (16, 6, 3, 3, 1), (24, 16, 3, 1, 1)):
        assert L.fiber_dcn_dx_bf16(P(dcols), None, None, P(dxb), P(ws), 1, 16, 16, C, Ho, Ho, k, k, st, pad, s) == 1, (C, Ho, k, st, pad)
    torch.cuda.synchronize()
    for i, b in enumerate(outs):
        assert bool(_nan(b).all()), f"buffer {i} written by a refused call"


# ---- launched kernels ------------------------------------------------------------------------------------------------------------------------
def test_dcn_paths_probe_names_the_declared_kernels():
    """tools/probes/dcn_optim_paths.py runs every case once under torch.profiler in a child: each launched the kernels it declares
    (which dcn_scatter_kernel<G> included), and nothing else."""
    r = run_bounded([sys.executable, os.path.join(ROOT, "tools", "probes", "dcn_optim_paths.py"), "dcn"], 300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    seen = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert set(seen) == set(dc.CASE_BY_NAME), sorted(set(dc.CASE_BY_NAME) ^ set(seen))
    wrong = {n: (dc.expected_kernels(dc.CASE_BY_NAME[n]), k) for n, k in seen.items() if dc.expected_kernels(dc.CASE_BY_NAME[n]) != k}
    assert not wrong, wrong
    assert {k for v in seen.values() for k in v if "scatter" in k} == {f"dcn_scatter_kernel<{g}>" for g in (1, 2, 4, 8, 16, 32, 64)}
