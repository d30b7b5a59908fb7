"""Launch pattern for counter passes on gemm_nt_q8_kernel (tools/pmc_q8_loop.sh): 20 launches of Y = X W^T + bias at one shape, randn operands.
    python tools/probes/pmc_q8.py M N K        (FIBER_HIP_LIB selects the library, as everywhere)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from fiber_amd import lib, ops

lib.load()
M, N, K = (int(v) for v in sys.argv[1:4])
x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
w = (torch.randn(N, K, device="cuda") * K ** -0.5).to(torch.bfloat16)
b = torch.randn(N, device="cuda")
for _ in range(20):
    ops.gemm_nt(x, w, b)
torch.cuda.synchronize()
print("flops per launch:", 2 * M * N * K, "K tiles per launch (all waves):", -(-M // 256) * -(-N // 256) * (K // 64) * 8)
