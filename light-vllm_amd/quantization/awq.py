"""AWQ (4-bit group-quantised weights, 16-bit activations) of the reference
(light_vllm/backends/quantization/awq.py): the config, the load-time repack for the gfx950 kernels
(csrc/awq_gemm.hip for decode, csrc/awq_tiled_gemm.hip for prefill), the linear, and a plain quantiser that produces
checkpoint-layout tensors."""
from typing import Any, Dict, List, Optional, Tuple

import torch

AWQ_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)  # nibble i of a packed word holds column 8 j + AWQ_ORDER[i]


class AWQConfig:
    """awq.py:12-63 of the reference."""

    def __init__(self, weight_bits: int, group_size: int, zero_point: bool) -> None:
        self.weight_bits = weight_bits
        self.group_size = group_size
        self.zero_point = zero_point
        if self.weight_bits != 4:
            raise ValueError("Currently, only 4-bit weight quantization is supported for "
                             f"AWQ, but got {self.weight_bits} bits.")
        self.pack_factor = 32 // self.weight_bits

    def __repr__(self) -> str:
        return (f"AWQConfig(weight_bits={self.weight_bits}, group_size={self.group_size}, "
                f"zero_point={self.zero_point})")

    def get_name(self) -> str:
        return "awq"

    def get_supported_act_dtypes(self) -> List[torch.dtype]:
        return [torch.half, torch.bfloat16]  # the reference's kernel is fp16 only

    @staticmethod
    def get_config_filenames() -> List[str]:
        return ["quant_config.json", "quantize_config.json"]

    @staticmethod
    def get_from_keys(config: Dict[str, Any], keys: List[str]) -> Any:
        for key in keys:
            if key in config:
                return config[key]
        raise ValueError(f"Cannot find any of {keys} in the model's quantization config.")

    @classmethod
    def from_config(cls, config: Dict[str, Any]) -> "AWQConfig":
        weight_bits = cls.get_from_keys(config, ["w_bit", "bits"])
        group_size = cls.get_from_keys(config, ["q_group_size", "group_size"])
        zero_point = cls.get_from_keys(config, ["zero_point"])
        return cls(weight_bits, group_size, zero_point)


def _pack_nibbles(v: torch.Tensor) -> torch.Tensor:
    """[R, N] integers 0..15 -> int32 [R, N/8] in the checkpoint's nibble order."""
    R, N = v.shape
    v = v.to(torch.int64).reshape(R, N // 8, 8)
    word = torch.zeros(R, N // 8, dtype=torch.int64, device=v.device)
    for i, col in enumerate(AWQ_ORDER):
        word |= v[:, :, col] << (4 * i)
    return torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32)


def quantize_awq(weight: torch.Tensor, group_size: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """weight [N, K] -> (qweight int32 [K, N/8], qzeros int32 [K/G, N/8], scales [K/G, N]) in the checkpoint layout
    (awq.py:103-151, nibble interleave of quant_utils.py:374-391).  Plain asymmetric round-to-nearest per group of
    `group_size` input channels: s = (max - min) / 15, z = round(-min / s), q = clamp(round(w / s) + z, 0, 15),
    with two guards: the group's range is widened to hold 0 (min <= 0 <= max), so that z stays within 0..15, and s is
    multiplied by (1 + eps of the weight's dtype) before it is rounded to that dtype, so that the stored scale is
    never below the exact one and 15 steps still span the range (every element then lies within s / 2).
    It does NO activation-aware scaling search -- it is how the engine and the tests obtain AWQ tensors where no
    checkpoint exists, not a substitute for the AWQ algorithm."""
    N, K = weight.shape
    assert K % group_size == 0 and N % 8 == 0
    w = weight.double().t().reshape(K // group_size, group_size, N)  # [groups, G, N]
    lo, hi = w.amin(dim=1).clamp(max=0), w.amax(dim=1).clamp(min=0)  # the range holds 0, so that z is 0..15
    # the scale as the kernels will see it, rounded to the weight's dtype from above: 15 steps still span the range
    scales = ((hi - lo) / 15 * (1 + torch.finfo(weight.dtype).eps)).clamp_min(1e-5).to(weight.dtype)
    s = scales.double()
    z = torch.round(-lo / s).clamp(0, 15)
    q = (torch.round(w / s[:, None, :]) + z[:, None, :]).clamp(0, 15)
    return _pack_nibbles(q.reshape(K, N)), _pack_nibbles(z), scales.contiguous()


def pack_awq_weight(qweight: torch.Tensor, qzeros: torch.Tensor, scales: torch.Tensor):
    """Checkpoint tensors -> (w4_packed, meta) in the order the streaming kernel reads; once, after loading."""
    return torch.ops._C_amd.awq_pack(qweight, qzeros, scales)


def apply_awq_linear(x: torch.Tensor, w4_packed: torch.Tensor, meta: torch.Tensor, qweight: torch.Tensor,
                     qzeros: torch.Tensor, scales: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """awq.py:153-175 of the reference, on the packed pair for every row count: skinny_linear_w4a16 decides the route
    (the streaming kernel for decode batches of <= 64 rows, the LDS-tiled kernel for prefill batches inside the tuning
    range w4_tiled_min_rows .. w4_tiled_max_rows, dequantise-from-packed + library GEMM elsewhere).  The checkpoint
    tensors only give the shape here."""
    K, N = qweight.shape[0], scales.shape[1]
    out = torch.ops._C_amd.skinny_linear_w4a16(x.reshape(-1, K), w4_packed, meta, N, K, K // scales.shape[0], bias)
    return out.reshape(x.shape[:-1] + (N,))
