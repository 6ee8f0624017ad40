"""quantization="int8" through the engine: Weight.quantize_int8 + linear() against apply_int8_linear's arithmetic
restated in torch, and the tiny model end to end (eager == HIP graph, tokens inside the vocabulary, fewer weight bytes
than the 16-bit model, lm_head still 16-bit).  Every projection of the tiny model (hidden 256, intermediate 512) is
inside the kernel's envelope, so the model runs the packed streaming kernel, not the fallback; the fallback is the
second weight of the first test."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("rows", [8, 100])
@pytest.mark.parametrize("N,K,packs", [(96, 256, True), (24, 96, False)])
def test_weight_quantize_int8_and_linear(ops, rows, N, K, packs):
    from light_vllm_amd.engine.model import Weight, linear
    from light_vllm_amd.quantization import quantize_int8_weight
    g = torch.Generator(device=DEV).manual_seed(rows)
    w16 = (torch.randn(N, K, generator=g, device=DEV) * 0.05).to(torch.bfloat16)
    w = Weight(w16)
    w.quantize_int8()
    assert w.w is None and w.packed is None and (w.i8_packed is not None) == packs and (w.i8 is None) == packs
    assert w.nbytes() == N * K + 4 * N
    x = (torch.randn(rows, K, generator=g, device=DEV) * 0.5).to(torch.bfloat16)
    wq, sw = (t.cpu() for t in quantize_int8_weight(w16))
    xf = x.cpu().float()  # the reference on the CPU: IEEE fp32 division and multiplication
    a = xf.abs().amax(dim=1, keepdim=True)
    c127 = torch.full_like(a, 127.0)
    xq = torch.round(xf * (c127 / a)).clamp(-128, 127)
    acc = (xq.double() @ wq.double().t()).float()  # exact integers
    ref = ((a / c127) * (sw[None, :] * acc)).to(torch.bfloat16)
    assert torch.equal(linear(x, w).cpu(), ref)


def make_engine(graph, quantization):
    from light_vllm_amd.engine.config import CacheConfig, ModelConfig, SchedulerConfig
    from light_vllm_amd.engine.llm_engine import LLMEngine
    cfg = ModelConfig.tiny()
    cfg.quantization = quantization
    return LLMEngine(cfg, CacheConfig(block_size=16, num_gpu_blocks=256, num_cpu_blocks=32),
                     SchedulerConfig(max_num_batched_tokens=2048, max_num_seqs=8, max_model_len=512),
                     device=DEV, use_hip_graph=graph, seed=0)


def run_to_completion(engine, max_tokens=8):
    g = torch.Generator().manual_seed(0)
    ps = [torch.randint(0, 512, (n,), generator=g).tolist() for n in (5, 37, 16, 1)]
    for i, p in enumerate(ps):
        engine.add_request(str(i), p, max_tokens=max_tokens)
    final = {}
    for _ in range(200):
        for out in engine.step():
            if out.finished:
                final[out.request_id] = out.token_ids
        if not engine.has_unfinished_requests():
            break
    engine.shutdown()
    return [final[str(i)] for i in range(len(ps))]


def test_int8_engine_runs_to_completion():
    e = make_engine(False, "int8")
    model = e.worker.model
    assert all(w.i8_packed is not None and w.w is None for l in model.layers for w in (l.qkv, l.o, l.gate_up, l.down))
    assert model.lm_head.i8_scale is None and model.lm_head.packed is not None
    int8_bytes = model.weight_bytes()
    eager = run_to_completion(e)
    graph = run_to_completion(make_engine(True, "int8"))
    assert eager == graph
    assert all(len(t) == 8 and all(0 <= tok < 512 for tok in t) for t in eager)
    e16 = make_engine(False, None)
    assert int8_bytes < e16.worker.model.weight_bytes()
    e16.shutdown()
