"""int8 helpers that need no GPU: the per-channel weight quantiser's round trip."""
import torch


def test_quantize_int8_weight_round_trip_within_half_a_step():
    from light_vllm_amd.quantization import quantize_int8_weight
    w = (torch.randn(48, 200, generator=torch.Generator().manual_seed(0)) * 0.05).to(torch.bfloat16)
    w[5] = 0
    q, s = quantize_int8_weight(w)
    assert q.shape == (48, 200) and q.dtype == torch.int8 and s.shape == (48,) and s.dtype == torch.float32
    assert torch.equal(s, (w.double().abs().amax(dim=1) / 127).float()) and q.abs().max().item() == 127
    # |w - s q| <= s / 2 for the stored s, evaluated in float64 (1e-12: that evaluation's own rounding)
    err = (w.double() - s.double()[:, None] * q.double()).abs()
    assert (err <= s.double()[:, None] / 2 * (1 + 1e-12)).all()
    assert s[5].item() == 0.0 and q[5].count_nonzero().item() == 0
