"""W8A8 int8 (compressed-tensors / SmoothQuant) of the reference (backends/quantization/utils/w8a8_utils.py:192-209):
int8 weights with one fp32 scale per output channel, int8 activations with one fp32 scale per token (dynamic) or one
per tensor (static), int32 accumulation, out = x_scale[m] * (w_scale[n] * acc) + bias.  Activation quantisation and
the GEMM are this package's HIP kernels (csrc/int8_quant.hip, csrc/int8_gemm.hip)."""
from typing import Optional, Tuple

import torch

from .. import _custom_ops as ops


def quantize_int8_weight(weight: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[N, K] weight -> (w_q int8 [N, K], w_scale fp32 [N]): symmetric per output channel, s = max|w_n| / 127,
    q = clamp(rint(w / s), -127, 127); every element then lies within s / 2 of s * q.  An all-zero row gets
    scale 0 and zeros."""
    w = weight.double()  # the quotient in float64, against the scale as it is stored: the s / 2 bound is then exact
    s = (w.abs().amax(dim=1) / 127.0).float()
    q = torch.round(w / torch.where(s > 0, s, torch.ones_like(s)).double()[:, None]).clamp_(-127, 127)
    return q.to(torch.int8), s


def pack_int8_weight(w_q: torch.Tensor) -> torch.Tensor:
    """[N, K] int8 (row-major, N % 16 == 0, K % 64 == 0) -> the order the weight-streaming kernel reads, as a flat
    tensor of N * K bytes: one contiguous KiB per (16-row n-tile, 64-wide k-step)."""
    return torch.ops._C_amd.int8_pack(w_q.contiguous()).reshape(-1)


def apply_int8_linear(input: torch.Tensor, weight: torch.Tensor, weight_scale: torch.Tensor,
                      input_scale: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """w8a8_utils.py:192-209 of the reference.  input_scale None: dynamic per-token activation scales; a scalar
    tensor: static per-tensor.  `weight` is either the flat packed form of pack_int8_weight (with a per-channel
    weight_scale of N elements, which gives N) or, as the reference passes it, the [K, N] transpose of the row-major
    int8 weight, which goes through cutlass_scaled_mm (packed per call inside the kernel's envelope, an exact float64
    matmul outside)."""
    K = input.shape[-1]
    x_q, x_scale = ops.scaled_int8_quant(input.reshape(-1, K), input_scale)
    if weight.dim() == 1:
        N = weight_scale.numel()
        assert weight.numel() == N * K, "packed weight: weight_scale must hold one scale per output channel"
        out = torch.ops._C_amd.skinny_linear_w8a8_int8(x_q, weight, x_scale, weight_scale, N, K, bias, input.dtype)
    else:
        N = weight.shape[1]
        out = ops.cutlass_scaled_mm(x_q, weight, scale_a=x_scale, scale_b=weight_scale, out_dtype=input.dtype,
                                    bias=bias)
    return out.reshape(input.shape[:-1] + (N,))
