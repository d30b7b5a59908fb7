"""Which kernels each case of the deformable-convolution and optimizer path matrices (tests/dcn_cases.py, tests/optim_cases.py) launches:
every case once under torch.profiler (device activity only), after one untraced call, printed as one JSON line {case: [kernel, ...]}.
tests/test_hip_dcn_paths.py and tests/test_hip_optim_paths.py run this in a child process under a deadline and check each case against
the kernels it declares (which dcn_scatter_kernel<G> included).
    python tools/probes/dcn_optim_paths.py [dcn | optim]"""
import json
import os
import re
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from torch.profiler import ProfilerActivity, profile
from fiber_amd import lib
from tests import dcn_cases as dc
from tests import optim_cases as oc

torch.cuda.set_device(0)
lib.load()
which = sys.argv[1:] or ["dcn", "optim"]


def demangle(name):
    """'_ZN12_GLOBAL__N_118dcn_scatter_kernelILi8EEEv...' -> 'dcn_scatter_kernel<8>' (the profiler reports some kernels mangled)"""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", name)
    if not m:
        return name
    i = m.end()
    n = int(m.group(1))
    base, rest = name[i:i + n], name[i + n:]
    if not rest.startswith("I"):
        return base
    args = [val for _k, val in re.findall(r"L([ib])(\d+)E", rest[1:rest.index("EE") + 1])]
    return f"{base}<{', '.join(args)}>"


def short(name):
    name = demangle(name)
    name = re.sub(r"^void ", "", name).replace("(anonymous namespace)::", "")
    return name.split("(")[0]


def traced(fn):
    fn()                                                     # (first call: library loads outside the trace)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = {short(e.name) for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name
             and "Memset" not in e.name and "fillBuffer" not in e.name and "copyBuffer" not in e.name}
    return sorted(k for k in names if not k.startswith("at::"))     # (the fills of the output buffers are torch kernels)


seen = {}
if "dcn" in which:
    run = {"gather": dc.run_gather, "scatter": dc.run_scatter, "tiled": dc.run_tiled}
    for case in dc.CASES:
        dev = dc.to_device(dc.make_inputs(case))
        want = ("dx",) if case["kind"] == "scatter" and case["off"] is None else None
        seen[case["name"]] = traced((lambda: dc.run_scatter(lib, case, dev, want)) if want else (lambda: run[case["kind"]](lib, case, dev)))
if "optim" in which:
    for case in oc.ADAM_CASES:
        st = oc.make_state(case)
        seen[f"adam:{case['name']}"] = traced(lambda: oc.run_adam(lib, case, st))
    for k in oc.DESC_SETS:
        seen[f"transpose:{k}"] = traced(lambda: oc.run_transpose(lib, k))
    for k in oc.PERM_SETS:
        seen[f"rowperm:{k}"] = traced(lambda: oc.run_rowperm(lib, k))
print(json.dumps(seen), flush=True)
