"""Which kernel each case of the NT GEMM path matrix (tests/gemm_cases.py) launches: every case once under torch.profiler (device
activity only), printed as one JSON line {case: [kernel names]}.  tests/test_hip_gemm_paths.py runs this in a child process under a
deadline and checks each case against the template it declares.
    python tools/probes/gemm_paths.py [case ...]"""
import json
import os
import re
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from torch.profiler import ProfilerActivity, profile
from fiber_amd import lib, ops
from tests import gemm_cases as gc

torch.cuda.set_device(0)
lib.load()
names = sys.argv[1:] or [c["name"] for c in gc.CASES]


def short(name):
    """'void (anonymous namespace)::gemm_nt_q8_kernel<0, true, true, false>((anonymous namespace)::GemmArgs)' -> the template id"""
    name = re.sub(r"^void ", "", name).replace("(anonymous namespace)::", "")
    return name.split("(")[0]


seen = {}
for n in names:
    case = gc.CASE_BY_NAME[n]
    inp = gc.make_inputs(case)
    gc.run(ops, case, inp)                                   # (first call: library loads and one-time attributes outside the trace)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        gc.run(ops, case, inp)
        torch.cuda.synchronize()
    seen[n] = sorted({short(e.name) for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name
                      and "Memset" not in e.name and "fillBuffer" not in e.name and "copyBuffer" not in e.name})
    del inp
print(json.dumps(seen), flush=True)
