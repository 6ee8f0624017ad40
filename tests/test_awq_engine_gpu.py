"""quantization="awq" through the engine: Weight.quantize_awq + linear() against x @ Wd, and the tiny model end to
end (eager == HIP graph, tokens inside the vocabulary, fewer weight bytes than the 16-bit model)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("rows", [8, 100])
def test_weight_quantize_awq_and_linear(ops, rows):
    from light_vllm_amd.engine.model import Weight, linear
    g = torch.Generator(device=DEV).manual_seed(rows)
    w = Weight((torch.randn(96, 256, generator=g, device=DEV) * 0.05).to(torch.bfloat16))
    w.quantize_awq(64)
    assert w.w is None and w.packed is None and w.w4_packed is not None
    x = (torch.randn(rows, 256, generator=g, device=DEV) * 0.5).to(torch.bfloat16)
    qweight, qzeros, scales = w.awq

    def unpack(words):  # nibble i of word j is column 8 j + [0,2,4,6,1,3,5,7][i]
        out = torch.empty(words.shape[0], 96, dtype=torch.int64, device=DEV)
        for i, c in enumerate([0, 2, 4, 6, 1, 3, 5, 7]):
            out[:, c::8] = (words.to(torch.int64) >> (4 * i)) & 15
        return out

    wd = ((unpack(qweight) - unpack(qzeros).repeat_interleave(64, 0)).float()
          * scales.float().repeat_interleave(64, 0)).to(torch.bfloat16)
    ref = x.float() @ wd.float()
    y = linear(x, w)
    assert y.shape == (rows, 96)
    assert (y.float() - ref).abs().max().item() <= 2 ** -7 * ref.abs().max().item() + 1e-3


def make_engine(graph, quantization):
    from light_vllm_amd.engine.config import CacheConfig, ModelConfig, SchedulerConfig
    from light_vllm_amd.engine.llm_engine import LLMEngine
    cfg = ModelConfig.tiny()
    cfg.quantization = quantization
    cfg.awq_group_size = 128
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


def test_awq_engine_runs_to_completion():
    e = make_engine(False, "awq")
    layer = e.worker.model.layers[0]
    assert all(w.w4_packed is not None and w.w is None for w in (layer.qkv, layer.o, layer.gate_up, layer.down))
    assert e.worker.model.lm_head.w4_packed is None and e.worker.model.lm_head.packed is not None
    awq_bytes = e.worker.model.weight_bytes()
    eager = run_to_completion(e)
    graph = run_to_completion(make_engine(True, "awq"))
    assert eager == graph
    assert all(len(t) == 8 and all(0 <= tok < 512 for tok in t) for t in eager)
    e16 = make_engine(False, None)
    assert awq_bytes < e16.worker.model.weight_bytes()
    e16.shutdown()
