"""The LDS-tiled W4A8 MXFP4 kernel through the engine: linear(x, Weight) above tuning mxfp4_tiled_min_rows against
float64 on the exact activation grid of test_mxfp4_engine_gpu.py, and the tiny quantization="mxfp4" model with every
projection call, prompt and decode alike, on the tiled kernel (eager == HIP graph, tokens inside the vocabulary)."""
import pytest
import torch

from test_int8_engine_gpu import make_engine, run_to_completion

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def min_rows(ops):
    get, put = torch.ops._C_amd.get_tuning, torch.ops._C_amd.set_tuning
    rows = get("mxfp4_tiled_min_rows")
    yield lambda v: put("mxfp4_tiled_min_rows", v)
    put("mxfp4_tiled_min_rows", rows)


def test_linear_takes_the_tiled_kernel(ops, min_rows):
    from light_vllm_amd.engine.model import Weight, linear
    from light_vllm_amd.quantization import dequantize_mxfp4, quantize_mxfp4_weight
    rows, N, K = 300, 96, 256
    g = torch.Generator(device=DEV).manual_seed(rows)
    w16 = (torch.randn(N, K, generator=g, device=DEV) * 0.05).to(torch.bfloat16)
    w = Weight(w16)
    w.quantize_mxfp4()
    wd = dequantize_mxfp4(*quantize_mxfp4_weight(w16), torch.float64).cpu()
    # multiples of 1/8 with max|row| = 1.75: the per-token scale is 2^-8 and the quantisation exact, every fp32 partial
    # sum exact in any order (test_weight_quantize_mxfp4_and_linear)
    x = torch.randint(-14, 15, (rows, K), generator=g, device=DEV).float() / 8
    x[:, 0] = 1.75
    x = x.to(torch.bfloat16)
    xq, sx = ops.scaled_fp8_quant(x, use_per_token_if_dynamic=True)
    assert (sx == 2.0 ** -8).all() and torch.equal(xq.float() * 2.0 ** -8, x.float())
    ref = ((xq.cpu().double() @ wd.t()) * sx.cpu().double()).to(torch.bfloat16)
    min_rows(65)
    assert torch.equal(linear(x, w).cpu(), ref)
    assert torch.equal(torch.ops._C_amd.linear_w4a8_mxfp4_tiled(xq, w.mx4_packed, w.mx4_scale, sx, N, K, None,
                                                                torch.bfloat16).cpu(), ref)


def test_mxfp4_engine_on_the_tiled_kernel(min_rows):
    min_rows(1)
    eager = run_to_completion(make_engine(False, "mxfp4"))
    graph = run_to_completion(make_engine(True, "mxfp4"))
    assert eager == graph
    assert all(len(t) == 8 and all(0 <= tok < 512 for tok in t) for t in eager)
