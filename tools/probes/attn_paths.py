"""Which kernels each case of the attention path matrix (tests/attn_cases.py) launches: every case's forward and backward once under
torch.profiler (device activity only), after one untraced call, printed as one JSON line {case: {"fwd": [...], "bwd": [...]}}.
tests/test_hip_attn_paths.py runs this in a child process under a deadline and checks each case against the kernels it declares.
    python tools/probes/attn_paths.py [case ...]"""
import json
import os
import re
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from torch.profiler import ProfilerActivity, profile
from fiber_amd import lib
from tests import attn_cases as ac

torch.cuda.set_device(0)
lib.load()
names = sys.argv[1:] or [c["name"] for c in ac.CASES]


def short(name):
    """'void (anonymous namespace)::t2i_fwd_kernel<false, true>((anonymous namespace)::FP)' -> the template id"""
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
    case = ac.CASE_BY_NAME[n]
    if case["kind"] == "window":
        inp = ac.make_window_inputs(case)
        o, lse = ac.run_window_fwd(lib, case, inp)
        fwd = traced(lambda: ac.run_window_fwd(lib, case, inp))
        bwd = traced(lambda: ac.run_window_bwd(lib, case, inp, o, lse, case["colsum"]))
    else:
        inp = ac.make_mha_inputs(case)
        o, lse = ac.run_mha_fwd(lib, case, inp)
        fwd = traced(lambda: ac.run_mha_fwd(lib, case, inp))
        bwd = traced(lambda: ac.run_mha_bwd(lib, case, inp, o, lse))
    seen[n] = {"fwd": fwd, "bwd": bwd}
    del inp
print(json.dumps(seen), flush=True)
