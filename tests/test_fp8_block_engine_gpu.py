"""quantization="fp8_block" through the engine: Weight.quantize_fp8_block + linear() against the arithmetic restated
in float64, the weight quantiser's error bound, and the tiny model end to end (eager == HIP graph, tokens inside the
vocabulary, every layer projection packed, lm_head still 16-bit, fewer weight bytes than the 16-bit model)."""
import pytest
import torch

from test_int8_engine_gpu import make_engine, run_to_completion

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("rows", [8, 100])
@pytest.mark.parametrize("N,K,packs", [(160, 256, True), (24, 96, False)])
def test_weight_quantize_fp8_block_and_linear(ops, rows, N, K, packs):
    from light_vllm_amd.engine.model import Weight, linear
    from light_vllm_amd.quantization import dequantize_fp8_block, quantize_fp8_block_weight
    g = torch.Generator(device=DEV).manual_seed(rows)
    # weights and activations on grids that both quantisers map exactly.  W: multiples of 1/64 with every block's max
    # 14/64, so the block scale is 2^-11 and the fp8 values are multiples of 32 of at most 4 significant bits.  X:
    # multiples of 1/8 with every group's max 1.75, so the group scale is 2^-8 and the fp8 values likewise.  Products
    # are multiples of 2^10 summing far below 2^24 of them: fp32 accumulation is exact in any order, and the scale
    # product a power of two
    w16 = torch.randint(-14, 15, (N, K), generator=g, device=DEV).float() / 64
    w16[::128, ::128] = 14 / 64
    w = Weight(w16.to(torch.bfloat16))
    w.quantize_fp8_block()
    assert w.w is None and w.packed is None and (w.f8b_packed is not None) == packs and (w.f8b is None) == packs
    assert w.nbytes() == N * K + 4 * w.f8b_scale.numel() and w.f8b_scale.shape == ((N + 127) // 128, (K + 127) // 128)
    wq, ws = quantize_fp8_block_weight(w16.to(torch.bfloat16))
    assert (ws == 2.0 ** -11).all() and torch.equal(dequantize_fp8_block(wq, ws), w16)
    x = torch.randint(-14, 15, (rows, K), generator=g, device=DEV).float() / 8
    x[:, ::128] = 1.75
    ref = (x.cpu().double() @ w16.cpu().double().t()).to(torch.bfloat16)
    y = linear(x.to(torch.bfloat16), w).cpu()
    assert y.dtype == torch.bfloat16
    if packs:
        assert torch.equal(y, ref)
    else:  # the library's fp32 matmul: its own summation, one bf16 ulp
        assert ((y.double() - ref.double()).abs() <= 2.0 ** (torch.floor(torch.log2(ref.double().abs().clamp_min(2.0 ** -126))) - 7)).all()


def test_weight_quantiser_is_within_half_an_e4m3_step():
    from light_vllm_amd.quantization import dequantize_fp8_block, quantize_fp8_block_weight
    w = (torch.randn(200, 300, generator=torch.Generator().manual_seed(0)) * 0.05).to(torch.bfloat16)
    wq, ws = quantize_fp8_block_weight(w)
    assert wq.shape == (200, 300) and ws.shape == (2, 3)
    s = ws.double().repeat_interleave(128, dim=0)[:200].repeat_interleave(128, dim=1)[:, :300]
    v = w.double() / s  # e4m3 step at v: 2^(floor(log2 |v|) - 3), 2^-9 below 2^-6; the fp32 division adds 2^-24 |v|
    step = 2.0 ** (torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -6))) - 3)
    assert ((dequantize_fp8_block(wq, ws, torch.float64) - w.double()).abs() <= (step / 2 + 2.0 ** -23 * v.abs()) * s).all()
    assert (wq.float().abs().view(-1) <= 448).all()


def test_fp8_block_engine_runs_to_completion():
    e = make_engine(False, "fp8_block")
    model = e.worker.model
    assert all(w.f8b_packed is not None and w.w is None for l in model.layers for w in (l.qkv, l.o, l.gate_up, l.down))
    assert model.lm_head.f8b_scale is None and model.lm_head.packed is not None
    f8_bytes = model.weight_bytes()
    eager = run_to_completion(e)
    graph = run_to_completion(make_engine(True, "fp8_block"))
    assert eager == graph
    assert all(len(t) == 8 and all(0 <= tok < 512 for tok in t) for t in eager)
    e16 = make_engine(False, None)
    assert f8_bytes < e16.worker.model.weight_bytes()
    e16.shutdown()
