"""fp8 W8A8 linear of the reference (backends/quantization/utils/w8a8_utils.py): activation
quantisation by this package's HIP kernels, GEMM + dequantisation through `torch._scaled_mm`
(hipBLASLt fp8 MFMA on gfx950, OCP e4m3fn) -- the reference's own route on ROCm, where its CUTLASS
kernels do not exist.  AWQ W4A16 (backends/quantization/awq.py): load-time repack and the gfx950
weight-streaming kernel with in-register dequantisation.  W8A8 int8 (w8a8_utils.py:192-209): per-token activation
quantisation and the int32-accumulating weight-streaming kernel, where the reference calls CUTLASS.  W4A8 MXFP4 (OCP microscaling; not in the
reference): fp4 weights with E8M0 block scales streamed into gfx950's scaled MFMA against fp8 activations.  Block-scaled
W8A8 fp8 (the DeepSeek-V3 / Qwen3 "-FP8" checkpoint format; not in the reference): one fp32 scale per 128 x 128 weight
block and per token and 128 input channels, applied to each k-step's partial tile between MFMAs."""
from .awq import AWQConfig, apply_awq_linear, pack_awq_weight, quantize_awq  # noqa: F401
from .fp8 import (apply_fp8_linear, pack_fp8_weight, per_tensor_quantize_weight,  # noqa: F401
                  skinny_fp8_linear)
from .fp8_block import (apply_fp8_block_linear, dequantize_fp8_block, pack_fp8_block_weight,  # noqa: F401
                        quantize_fp8_block_weight)
from .int8 import apply_int8_linear, pack_int8_weight, quantize_int8_weight  # noqa: F401
from .mxfp4 import (apply_mxfp4_linear, dequantize_mxfp4, pack_mxfp4_weight,  # noqa: F401
                    quantize_mxfp4_weight)
