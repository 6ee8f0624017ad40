"""Kernel times of the block-scaled W8A8 fp8 decode launch and the per-tensor W8A8 launch at one (shape, M), for
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/trace_fp8_block.py qkv 1
The two kernels show up by name (skinny_gemm_fp8_block_kernel, the per-tensor skinny_gemm kernel); the difference
between a kernel's time here and the device-event time of tools/bench_gemm.py --fp8-block is what the launch costs
outside the kernel.  Weights rotate through > 1 GB, as in the bench."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import light_vllm_amd  # noqa: F401
from light_vllm_amd import _custom_ops  # noqa: F401

SHAPES = {"qkv": (6144, 4096), "o": (4096, 4096), "gate_up": (28672, 4096), "down": (4096, 14336)}
N, K = SHAPES[sys.argv[1]]
M = int(sys.argv[2]) if len(sys.argv) > 2 else 1
dev = "cuda:0"
w8 = torch.randint(0, 120, (N * K,), device=dev, dtype=torch.uint8)
nw = int(1.1e9 // (N * K)) + 1
wb, wt = [w8.clone() for _ in range(nw)], [w8.clone() for _ in range(nw)]
ws = torch.rand((N + 127) // 128, K // 128, device=dev) * 1e-2 + 1e-3
one = torch.ones(1, device=dev)
x16 = (torch.randn(M, K, device=dev) * 0.5).to(torch.bfloat16)
xq, xs = torch.ops._C_amd.per_token_group_fp8_quant(x16)
for i in range(300):
    torch.ops._C_amd.skinny_linear_w8a8_fp8_block(xq, wb[i % nw], xs, ws, N, K, None, torch.bfloat16)
    torch.ops._C_amd.skinny_linear_w8a8(x16, wt[i % nw], one, one, N, K, None)
torch.cuda.synchronize()
