"""Which kernels each case of the LayerNorm path matrix (tests/norm_cases.py) launches: every case's forward and backward once under
torch.profiler (device activity only), after one untraced call, printed as one JSON line {case: {"fwd": [...], "bwd": [...]}}.
tests/test_hip_norm_paths.py runs this in a child process under a deadline and checks each case against the kernels it declares.
    python tools/probes/norm_paths.py [case ...]"""
import json
import os
import re
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from torch.profiler import ProfilerActivity, profile
from fiber_amd import lib
from tests import norm_cases as nc

torch.cuda.set_device(0)
lib.load()
names = sys.argv[1:] or [c["name"] for c in nc.CASES]


def demangle(name):
    """'_ZN12_GLOBAL__N_113ln_fwd_kernelILi16ELi1ELb0ELb1ELi4EEEv...' -> 'ln_fwd_kernel<16, 1, false, true, 4>' (the profiler reports
    some of these kernels unmangled and some mangled; the templates here take only int and bool arguments)"""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", name)
    if not m:
        return name
    i = m.end()
    n = int(m.group(1))
    base, rest = name[i:i + n], name[i + n:]
    if not rest.startswith("I"):
        return base
    args = []
    for kind, val in re.findall(r"L([ib])(\d+)E", rest[1:rest.index("EE") + 1]):
        args.append(val if kind == "i" else ("true" if val == "1" else "false"))
    return f"{base}<{', '.join(args)}>"


def short(name):
    """'void (anonymous namespace)::ln_fwd_kernel<16, 1, false, false, 4>(void const*, ...)' -> the template id"""
    name = demangle(name)
    name = re.sub(r"^void ", "", name).replace("(anonymous namespace)::", "")
    return name.split("(")[0]


def traced(fn):
    fn()                                                     # (first call: library loads and one-time attributes outside the trace)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = {short(e.name) for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name
             and "Memset" not in e.name and "fillBuffer" not in e.name and "copyBuffer" not in e.name}
    return sorted(k for k in names if not k.startswith("at::"))     # (the NaN fills of the output buffers are torch kernels)


seen = {}
for n in names:
    case = nc.CASE_BY_NAME[n]
    if case["kind"] == "mlp":
        inp = nc.make_mlp_inputs(case)
        fwd = traced(lambda: nc.run_mlp_fwd(lib, case, inp))
        bwd = traced(lambda: nc.run_mlp_bwd(lib, case, inp))
    else:
        inp = nc.make_ln_inputs(case)
        f = nc.run_ln_fwd(lib, case, inp)
        fwd = traced(lambda: nc.run_ln_fwd(lib, case, inp))
        bwd = traced(lambda: nc.run_ln_bwd(lib, case, inp, f))
    seen[n] = {"fwd": fwd, "bwd": bwd}
    del inp
print(json.dumps(seen), flush=True)
