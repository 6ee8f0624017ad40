"""Block-scaled W8A8 fp8, the format DeepSeek-V3 / R1 and the Qwen3 "-FP8" checkpoints ship in: float8_e4m3fn weights
with one fp32 scale per 128 x 128 block, activations quantised on the fly to float8_e4m3fn with one fp32 scale per
token and 128 input channels (csrc/fp8_block_quant.hip, csrc/fp8_block_gemm.hip):
out[m, n] = sum_b xs[m, b] * ws[n // 128, b] * sum_{k in block b} xq[m, k] * wq[n, k] + bias[n]."""
from typing import Optional, Tuple

import torch

FP8_MAX = 448.0


def _block_view(t: torch.Tensor, block: int) -> torch.Tensor:
    """[N, K] -> [ceil(N/block), block, ceil(K/block), block], zero-padded"""
    N, K = t.shape
    nb, kb = -(-N // block), -(-K // block)
    p = torch.zeros(nb * block, kb * block, dtype=t.dtype, device=t.device)
    p[:N, :K] = t
    return p.view(nb, block, kb, block)


def quantize_fp8_block_weight(weight: torch.Tensor, block: int = 128) -> Tuple[torch.Tensor, torch.Tensor]:
    """[N, K] weight -> (wq [N, K] float8_e4m3fn, ws [ceil(N/block), ceil(K/block)] float32): the scale of a block is
    its absmax / 448 (1e-10 / 448 for an all-zero block), elements are divided by it and rounded to nearest even."""
    N, K = weight.shape
    w = _block_view(weight.float(), block)
    ws = w.abs().amax(dim=(1, 3)).clamp_min(1e-10) / FP8_MAX
    wq = (w / ws[:, None, :, None]).clamp(-FP8_MAX, FP8_MAX).reshape(w.shape[0] * block, -1)[:N, :K]
    return wq.to(torch.float8_e4m3fn).contiguous(), ws


def dequantize_fp8_block(wq: torch.Tensor, ws: torch.Tensor, dtype: torch.dtype = torch.float32,
                         block: int = 128) -> torch.Tensor:
    """(wq [N, K], ws [ceil(N/block), ceil(K/block)]) -> the [N, K] weight they stand for; exact in float64, rounded
    once to `dtype`."""
    N, K = wq.shape
    s = ws.double().repeat_interleave(block, dim=0)[:N].repeat_interleave(block, dim=1)[:, :K]
    return (wq.double() * s).to(dtype)


def pack_fp8_block_weight(wq: torch.Tensor) -> torch.Tensor:
    """[N, K] float8_e4m3fn (N % 16 == 0, K % 128 == 0) -> the flat byte order the streaming kernel reads: 2 contiguous
    KiB per (16-row n-tile, 128-wide k-step).  A pure permutation; the scales stay as they are."""
    return torch.ops._C_amd.fp8_block_pack(wq.contiguous())


def apply_fp8_block_linear(x: torch.Tensor, w: torch.Tensor, ws: torch.Tensor, N: int, K: int,
                           bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`w` is the flat tensor of pack_fp8_block_weight -- the HIP kernels, any number of rows -- or, for a weight
    outside the kernel's envelope (N % 16, K % 128), the 2-D wq, which is dequantised for the library matmul on
    activations quantised by the same per-group rule."""
    x2 = x.reshape(-1, K)
    if w.dim() == 1:
        xq, xs = torch.ops._C_amd.per_token_group_fp8_quant(x2)
        out = torch.ops._C_amd.skinny_linear_w8a8_fp8_block(xq, w, xs, ws, N, K, bias, x.dtype)
    else:
        g = torch.nn.functional.pad(x2.float(), (0, -K % 128)).view(x2.shape[0], -1, 128)  # [M, ceil(K/128), 128]
        xs = g.abs().amax(dim=2, keepdim=True).clamp_min(1e-10) / FP8_MAX
        xq = (g / xs).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).float()
        out = (xq * xs).reshape(x2.shape[0], -1)[:, :K] @ dequantize_fp8_block(w, ws).t()
        out = (out if bias is None else out + bias.float()).to(x.dtype)
    return out.reshape(x.shape[:-1] + (N,))
