"""Every optimizer kernel path through the C ABI with hand-built tables (tests/optim_cases.py): one AdamW launch over tensors of 1 ... 3 x 4096
elements at every gradient alignment, with p / m / v or the bf16 copy off their alignment (the scalar path), two tensors' chunks
interleaved; exp_avg, exp_avg_sq and p element by element against fp64, the bf16 copy equal to bf16 of the stored p to the bit, the
SENTINEL in front of and after every tensor untouched.  The transposed and the row-permuted bf16 copies to the bit, first to last tile of
every descriptor, guards after every destination.  FIBER_OPTIM_CALIBRATE=<file> records the largest value each constant needed."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import optim_cases as oc
from tests.hip_util import DEV, assert_elementwise
from tests.mp_util import run_bounded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONST = oc.CONST
_CAL = os.environ.get("FIBER_OPTIM_CALIBRATE")
_needed = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from fiber_amd import lib
    lib.load()
    return lib


def T64(a):
    return torch.from_numpy(np.array(a)).to(torch.float64)


def check(name, got, ref, c, term):
    got, ref, term = got.detach().cpu().to(torch.float64)[:, None], T64(ref)[:, None], T64(term)[:, None] * oc.F32
    if _CAL:
        need = (((got - ref).abs() - oc.TINY32) / term.clamp_min(1e-300)).where(term > 0, torch.zeros_like(ref)).max().item()
        if need > _needed.get(c, (0.0, ""))[0]:
            _needed[c] = (need, name)
        with open(_CAL, "w") as f:
            json.dump(_needed, f, indent=1)
    return assert_elementwise(name, got, ref, CONST[c] * term + oc.TINY32)


def assert_guards(name, buf, view):
    lead = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    rest = torch.cat([buf[:lead], buf[lead + view.numel():]])
    assert bool((rest == oc.SENTINEL).all()), f"{name}: an element outside the tensor was written"


@pytest.mark.parametrize("name", [c["name"] for c in oc.ADAM_CASES])
def test_adamw_path(lib, name):
    case = oc.ADAM_BY_NAME[name]
    assert all(CONST[k] <= oc.CEILING[k] for k in CONST)
    state = oc.make_state(case)
    bufs = oc.run_adam(lib, case, state)
    for i, (st, d) in enumerate(zip(state, bufs)):
        tag = f"{name} tensor {i} (n = {st['p'].size})"
        m1, v1, tm, tv = oc.moments_reference(case, st)
        check(f"{tag} exp_avg", d["m"], m1, "M", tm)
        check(f"{tag} exp_avg_sq", d["v"], v1, "V", tv)
        p1, tp = oc.param_reference(case, st["p"], d["m"].cpu().double().numpy(), d["v"].cpu().double().numpy())
        check(f"{tag} p", d["p"], p1, "P", tp)
        assert bool(torch.equal(d["g"].cpu(), torch.from_numpy(st["g"]))), f"{tag}: the gradient was written"
        for k in ("p", "m", "v", "g") + (("w",) if "w" in d else ()):
            assert_guards(f"{tag} {k}", d[k + "_buf"], d[k])
        if "w" in d:
            want = oc.bf16_bits(d["p"].cpu().numpy()).view(np.int16)
            assert np.array_equal(d["w"].view(torch.int16).cpu().numpy(), want), f"{tag}: bf16 copy is not bf16(p) of the stored p"


def test_adamw_hyper_words_override_the_arguments(lib):
    """the same step with the device words and wrong by-value lr / step gives the bits of the step with the right by-value arguments"""
    a, b = dict(oc.ADAM_BY_NAME["hyper"], hyper=False), oc.ADAM_BY_NAME["hyper"]
    st = oc.make_state(a)
    ra, rb = oc.run_adam(lib, a, st), oc.run_adam(lib, b, st)
    for i, (x, y) in enumerate(zip(ra, rb)):
        for k in ("p", "m", "v"):
            assert torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)), f"tensor {i} {k}"


def test_adamw_no_chunks_and_step_zero(lib):
    """nchunks = 0: FIBER_OK and nothing written; step = 0: FIBER_EINVAL and nothing written"""
    L, P = lib.load(), lib.ptr
    s = torch.cuda.current_stream().cuda_stream
    bufs = [torch.full((64,), oc.SENTINEL, device=DEV) for _ in range(4)]
    table = torch.tensor([[b.data_ptr() for b in bufs] + [0]], dtype=torch.int64).to(DEV)
    numel = torch.tensor([64], dtype=torch.int64).to(DEV)
    chunks = torch.tensor([[0, 0]], dtype=torch.int32).to(DEV)
    assert L.fiber_adamw_multi_f32(P(table), P(numel), P(chunks), 0, 1e-3, 0.01, 0.9, 0.98, 1e-8, 1, None, s) == 0
    assert L.fiber_adamw_multi_f32(P(table), P(numel), P(chunks), 1, 1e-3, 0.01, 0.9, 0.98, 1e-8, 0, None, s) == 1
    torch.cuda.synchronize()
    assert all(bool((b == oc.SENTINEL).all()) for b in bufs)


def _bits16(t):
    return t.view(torch.int16).cpu().numpy()


@pytest.mark.parametrize("which", list(oc.DESC_SETS))
def test_transpose_multi(lib, which):
    for i, (src, dst, N, K) in enumerate(oc.run_transpose(lib, which)):
        assert np.array_equal(_bits16(dst[:N * K]).reshape(K, N), _bits16(src).T), f"{which} descriptor {i} ({N} x {K})"
        assert bool((dst[N * K:].view(torch.int16) == -32768 + 0x7FC0).all()), f"{which} descriptor {i}: written past dst"


@pytest.mark.parametrize("which", list(oc.PERM_SETS))
def test_rowperm_cast_multi(lib, which):
    for i, d in enumerate(oc.run_rowperm(lib, which)):
        N, K, tag = d["N"], d["K"], f"{which} descriptor {i} ({d['N']} x {d['K']})"
        want = oc.bf16_bits(d["src"][d["perm"]]).view(np.int16)
        assert np.array_equal(_bits16(d["dst"][:N * K]).reshape(N, K), want), f"{tag}: dst"
        assert bool((d["dst"][N * K:].view(torch.int16) == -32768 + 0x7FC0).all()), f"{tag}: written past dst"
        if d["dst_t"] is not None:
            assert np.array_equal(_bits16(d["dst_t"][:N * K]).reshape(K, N), want.T), f"{tag}: dst_t"
            assert bool((d["dst_t"][N * K:].view(torch.int16) == -32768 + 0x7FC0).all()), f"{tag}: written past dst_t"
        bd = d["bias_dst"].view(torch.int32).cpu().numpy()
        if d["bias"] is not None:
            assert np.array_equal(bd[:N], d["bias"][d["perm"]].view(np.int32)), f"{tag}: bias"
            assert bool((bd[N:] == -4194304).all()), f"{tag}: written past bias_dst"
        else:
            assert bool((bd == -4194304).all()), f"{tag}: bias_dst written without a bias"


def test_optim_paths_probe_names_the_declared_kernels():
    r = run_bounded([sys.executable, os.path.join(ROOT, "tools", "probes", "dcn_optim_paths.py"), "optim"], 300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    seen = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert seen == oc.probe_cases(), (seen, oc.probe_cases())
