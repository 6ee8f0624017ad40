"""quantization="mxfp4" through the engine: Weight.quantize_mxfp4 + linear() against apply_mxfp4_linear's arithmetic
restated in torch, and the tiny model end to end (eager == HIP graph, tokens inside the vocabulary, fewer weight bytes
than the int8 model, lm_head still 16-bit).  Every projection of the tiny model (hidden 256, intermediate 512) is inside
the kernel's envelope, so the model runs the packed streaming kernel; the dequantising fallback is the second weight of
the first test."""
import pytest
import torch

from test_int8_engine_gpu import make_engine, run_to_completion

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("rows", [8, 100])
@pytest.mark.parametrize("N,K,packs", [(96, 256, True), (24, 96, False)])
def test_weight_quantize_mxfp4_and_linear(ops, rows, N, K, packs):
    from light_vllm_amd.engine.model import Weight, linear
    from light_vllm_amd.quantization import dequantize_mxfp4, quantize_mxfp4_weight
    g = torch.Generator(device=DEV).manual_seed(rows)
    w16 = (torch.randn(N, K, generator=g, device=DEV) * 0.05).to(torch.bfloat16)
    w = Weight(w16)
    w.quantize_mxfp4()
    assert w.w is None and w.packed is None and (w.mx4_packed is not None) == packs and (w.mx4 is None) == packs
    assert w.nbytes() == N * K // 2 + N * K // 32
    codes, scales = quantize_mxfp4_weight(w16)
    wd = dequantize_mxfp4(codes, scales, torch.float64).cpu()
    # the OCP rule: every element within half an e2m1 step (at most 2^e: the top binade's step is 2 * 2^e) of its
    # value, unless it saturated (max|block| up to 8 * 2^e against 6 * 2^e: within 2 * 2^e)
    step = torch.exp2(scales.cpu().double() - 127).repeat_interleave(32, dim=1)
    assert ((wd - w16.cpu().double()).abs() <= 2 * step).all() and (wd.abs() <= 6 * step).all()
    # activations on a grid that dynamic per-token quantisation maps exactly: multiples of 1/8 with max|row| = 1.75,
    # so the scale is 1.75 / 448 = 2^-8 and the fp8 values are multiples of 32 of at most 4 significant bits.  All
    # products are then multiples of 2^-3 times the smallest block scale and sum far below 2^24 of them: the fp32
    # accumulation is exact in any order and the scale product a power of two
    x = torch.randint(-14, 15, (rows, K), generator=g, device=DEV).float() / 8
    x[:, 0] = 1.75
    x = x.to(torch.bfloat16)
    xq, sx = ops.scaled_fp8_quant(x, use_per_token_if_dynamic=True)
    assert (sx == 2.0 ** -8).all() and torch.equal(xq.float() * 2.0 ** -8, x.float())
    ref = ((xq.cpu().double() @ wd.t()) * sx.cpu().double()).to(torch.bfloat16)
    y = linear(x, w).cpu()
    assert y.dtype == torch.bfloat16
    if packs:
        assert torch.equal(y, ref)
    else:  # the library's fp32 matmul: its own summation, one bf16 ulp
        assert ((y.double() - ref.double()).abs() <= 2.0 ** (torch.floor(torch.log2(ref.double().abs().clamp_min(2.0 ** -126))) - 7)).all()


def test_mxfp4_engine_runs_to_completion():
    e = make_engine(False, "mxfp4")
    model = e.worker.model
    assert all(w.mx4_packed is not None and w.w is None for l in model.layers for w in (l.qkv, l.o, l.gate_up, l.down))
    assert model.lm_head.mx4_scale is None and model.lm_head.packed is not None
    mx_bytes = model.weight_bytes()
    eager = run_to_completion(e)
    graph = run_to_completion(make_engine(True, "mxfp4"))
    assert eager == graph
    assert all(len(t) == 8 and all(0 <= tok < 512 for tok in t) for t in eager)
    e8 = make_engine(False, "int8")
    assert mx_bytes < e8.worker.model.weight_bytes()
    e8.shutdown()
