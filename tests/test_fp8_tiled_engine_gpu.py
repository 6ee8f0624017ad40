"""quantization="fp8" with the prompts' projections on the LDS-tiled fp8 kernel (csrc/fp8_tiled_gemm.hip): the row range
of apply_fp8_linear is forced open for the run, whatever the shipped defaults are."""
import pytest
import torch

from test_engine_gpu import collect_logits, make_engine

pytestmark = pytest.mark.gpu


def test_fp8_weights_engine_on_the_tiled_kernel_tracks_the_bf16_run(monkeypatch):
    """The assertion and the bound of test_fp8_weights_engine_tracks_the_bf16_run; the 213 prompt rows must not reach
    torch._scaled_mm."""
    get, put = torch.ops._C_amd.get_tuning, torch.ops._C_amd.set_tuning
    _, l16, _, _ = collect_logits(make_engine(graph=False), max_tokens=2)
    e8 = make_engine(graph=False, quantization="fp8")
    assert e8.worker.model.layers[0].qkv.w8_packed is not None
    lo, hi = get("fp8_tiled_min_rows"), get("fp8_tiled_max_rows")
    library_calls, scaled_mm = [], torch._scaled_mm
    monkeypatch.setattr(torch, "_scaled_mm", lambda *a, **k: library_calls.append(1) or scaled_mm(*a, **k))
    try:
        put("fp8_tiled_min_rows", 65)
        put("fp8_tiled_max_rows", 1 << 30)
        _, l8, _, _ = collect_logits(e8, max_tokens=2)
    finally:
        put("fp8_tiled_min_rows", lo)
        put("fp8_tiled_max_rows", hi)
    assert not library_calls
    for k in l16:
        a, b = l16[k][0], l8[k][0]  # first sampled position: same context in both runs
        cos = torch.nn.functional.cosine_similarity(a, b, dim=0).item()
        assert cos >= 0.97, (k, cos)
