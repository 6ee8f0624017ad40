"""W4A8 MXFP4: OCP microscaling fp4 weights (e2m1 elements, one E8M0 scale per 32 consecutive input channels of a
row) against fp8 e4m3fn activations, the format gfx950's scaled MFMA consumes as it is (csrc/mxfp4_gemm.hip):
out = x_scale[m] * sum_k x_q[m, k] * w4[n, k] * 2^(e[n, k/32] - 127) + bias.  Checkpoint layout: codes uint8
[N, K/2] (element k in byte k/2, even k in the low nibble), scales uint8 [N, K/32]."""
from typing import Optional, Tuple

import torch

from .. import _custom_ops as ops

# value of e2m1 code c (bit 3 the sign)
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0)


def quantize_mxfp4_weight(weight: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[N, K] weight (K % 32 == 0) -> (codes uint8 [N, K/2], scales uint8 [N, K/32]) by the OCP MX rule: the shared
    exponent of a block is floor(log2(max|block|)) - 2 (2 = e2m1's largest exponent), clamped to E8M0's finite codes;
    elements are divided by it, rounded to the nearest e2m1 value (ties to the even code) and saturate at +-6.  An
    all-zero block gets scale 127 and zeros."""
    N, K = weight.shape
    assert K % 32 == 0, "MX blocks are 32 consecutive input channels"
    w = weight.float().reshape(N, K // 32, 32)
    amax = w.abs().amax(dim=2, keepdim=True)
    _, ex = torch.frexp(amax)  # amax = m * 2^ex, 0.5 <= m < 1: floor(log2(amax)) = ex - 1
    e = torch.where(amax > 0, ex - 3, torch.zeros_like(ex)).clamp_(-127, 127)
    a = torch.ldexp(w.double(), -e).abs()  # exact
    # e2m1's grid: steps of 0.5 below 2, of 1 below 4, of 2 above; torch.round takes ties to even, which is the even code
    a = torch.where(a < 2, torch.round(a * 2) / 2, torch.where(a < 4, torch.round(a), torch.round(a / 2) * 2)).clamp_(max=6)
    code = torch.where(a < 2, a * 2, torch.where(a < 4, a + 2, a / 2 + 4)).to(torch.uint8)
    code = (code | ((w < 0).to(torch.uint8) << 3)).reshape(N, K // 2, 2)
    return code[..., 0] | (code[..., 1] << 4), (e + 127).to(torch.uint8).reshape(N, K // 32)


def dequantize_mxfp4(codes: torch.Tensor, scales: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """(codes [N, K/2], scales [N, K/32]) in checkpoint layout -> the [N, K] weight they stand for, in plain torch;
    exact in float64, rounded once to `dtype`."""
    N, K = codes.shape[0], codes.shape[1] * 2
    lut = torch.tensor(E2M1_VALUES, dtype=torch.float64, device=codes.device)
    idx = torch.stack((codes & 15, codes >> 4), dim=2).reshape(N, K // 32, 32).long()
    w = torch.ldexp(lut[idx], (scales.int() - 127)[..., None])
    return w.reshape(N, K).to(dtype)


def pack_mxfp4_weight(codes: torch.Tensor, scales: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Checkpoint layout (N % 16 == 0, K % 128 == 0) -> (w_packed, e_packed), flat uint8 tensors in the order the
    streaming kernel reads: one contiguous KiB of codes per (16-row n-tile, 128-wide k-step), one scale word per lane
    and four k-steps.  A scale of 0xFF (NaN) is refused."""
    return torch.ops._C_amd.mxfp4_pack(codes.contiguous(), scales.contiguous())


def apply_mxfp4_linear(x: torch.Tensor, w_packed: torch.Tensor, e_packed: torch.Tensor, N: int, K: int,
                       input_scale: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """input_scale None: dynamic per-token fp8 activation scales; a scalar tensor: static per-tensor.  `w_packed` /
    `e_packed` are the flat pair of pack_mxfp4_weight -- the HIP kernel, any number of rows -- or, for a weight
    outside the kernel's envelope (N % 16, K % 128), the 2-D checkpoint-layout pair, which is dequantised for the
    library matmul on the same quantised activations."""
    x_q, x_scale = ops.scaled_fp8_quant(x.reshape(-1, K), input_scale, use_per_token_if_dynamic=True)
    if w_packed.dim() == 1:
        out = torch.ops._C_amd.skinny_linear_w4a8_mxfp4(x_q, w_packed, e_packed, x_scale, N, K, bias, x.dtype)
    else:
        out = (x_q.float() @ dequantize_mxfp4(w_packed, e_packed).t()) * x_scale.reshape(-1, 1)
        out = (out if bias is None else out + bias.float()).to(x.dtype)
    return out.reshape(x.shape[:-1] + (N,))
