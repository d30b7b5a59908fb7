"""Which kernels each path of the element-wise, cross-entropy column-sum, embedding and im2col entry points launches (the paths of
tests/test_hip_ew_paths.py): every call once under torch.profiler (device activity only), after one untraced call, printed as one JSON
line {path: [kernel, ...]}.  tests/test_hip_ew_paths.py runs this in a child process under a deadline and checks every path.
    python tools/probes/ew_paths.py"""
import json
import os
import re
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from torch.profiler import ProfilerActivity, profile
from fiber_amd import lib

torch.cuda.set_device(0)
L = lib.load()
D, BF = "cuda", torch.bfloat16


def demangle(name):
    """'_ZN12_GLOBAL__N_117stream_add_kernelILi2EEEv...' -> 'stream_add_kernel<2>' (int and bool template arguments only)"""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", name)
    if not m:
        return name
    n = int(m.group(1))
    base, rest = name[m.end():m.end() + n], name[m.end() + n:]
    if not rest.startswith("I"):
        return base
    args = [v if k == "i" else ("true" if v == "1" else "false") for k, v in re.findall(r"L([ib])(\d+)E", rest[1:rest.index("EE") + 1])]
    return f"{base}<{', '.join(args)}>"


def short(name):
    name = re.sub(r"^void ", "", demangle(name)).replace("(anonymous namespace)::", "")
    return name.split("(")[0]


def traced(fn):
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = {short(e.name) for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name
             and "Memset" not in e.name and "fillBuffer" not in e.name and "copyBuffer" not in e.name}
    return sorted(k for k in names if not k.startswith("at::"))


def call(name, *args):
    rc = getattr(L, name)(*args, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (name, rc)


p = lambda t: t.data_ptr()
x = torch.randn(1 << 20, device=D).to(BF)
y = torch.empty(1 << 20, dtype=BF, device=D)
f = torch.rand(1 << 20, device=D)
o = torch.empty(1 << 20, device=D)
ws = torch.empty(1 << 20, device=D)
alpha = torch.tensor([0.5], device=D)
paths = {}
for kind, res in ((0, None), (1, p(x)), (2, p(f))):
    paths[f"stream_add res{kind}"] = lambda kind=kind, res=res: call("fiber_stream_add", res, kind, p(x), p(x), p(alpha), None, 0, 0.1, 1, 0.1, 2,
                                                                        None, p(o), p(y), 8192)
for tag, n in ((" 1 block", 2048), ("", 16384)):
    paths[f"stream_add_bwd dalpha{tag}"] = lambda n=n: call("fiber_stream_add_bwd", p(x), p(x), p(alpha), None, 0, 0.0, 0, 0.1, 3, None,
                                                            p(y), p(y), p(o), p(ws), n)
    paths[f"dot{tag}"] = lambda n=n: call("fiber_dot_bf16", p(x), p(x), p(o), p(ws), n)
for tag, M in (("", 64), (" slabs", 4096)):
    paths[f"colsum{tag}"] = lambda M=M: call("fiber_colsum_bf16", p(x), p(o), p(ws), M, 256, 256)
    paths[f"gelu_bwd_colsum{tag}"] = lambda M=M: call("fiber_gelu_bwd_colsum_bf16", p(x), p(x), p(y), p(o), p(ws), M, 256)
    paths[f"rowscale_colsum{tag}"] = lambda M=M: call("fiber_rowscale_colsum_bf16", p(x), p(f), p(y), p(o), p(ws), M, 256, 1)
lab = torch.where(torch.arange(600, device=D) % 3 == 0, 5, -100)
for tag, rows in (("", 64), (" slabs", 600)):
    paths[f"colsum_labelled{tag}"] = lambda rows=rows: call("fiber_colsum_labelled_bf16", p(x), p(lab), p(o), p(ws), rows, 1000, -100)
sel = torch.tensor([1, 0], dtype=torch.uint8, device=D)
paths["im2col"] = lambda: call("fiber_im2col_patch4", p(f), p(y), 2, 8, 8)
paths["im2col pair"] = lambda: call("fiber_im2col_patch4_pair", p(f), p(f), p(sel), p(y), 2, 8, 8)
B, S = 2, 8
ids = torch.randint(0, 50, (B, S), device=D)
pos = torch.empty(B * S, dtype=torch.int32, device=D)
mean, rstd = torch.empty(B * S, device=D), torch.empty(B * S, device=D)
tab = torch.randn(64 * 2048, device=D)
wsb = torch.empty(L.fiber_roberta_embed_bwd_workspace(B, S, 2048), device=D)
for C in (256, 512, 1024, 2048):
    paths[f"embed fwd C{C}"] = lambda C=C: call("fiber_roberta_embed_fwd", p(ids), p(tab), p(tab), p(tab), p(tab), p(tab), p(y), p(pos),
                                                p(mean), p(rstd), B, S, C, 1, 1e-5, 0.0, 0, None)
    paths[f"embed bwd C{C}"] = lambda C=C: call("fiber_roberta_embed_bwd", p(x), p(ids), p(pos), p(tab), p(tab), p(tab), p(tab), p(mean),
                                                p(rstd), p(ws), p(ws), p(o), p(o), p(o), p(wsb), B, S, C, 1, 0.0, 0, None)
seen = {}
for name, fn in paths.items():
    if name.startswith("embed bwd"):
        paths[name.replace("bwd", "fwd")]()                  # (pos / mean / rstd of this width)
    seen[name] = traced(fn)
print(json.dumps(seen), flush=True)
