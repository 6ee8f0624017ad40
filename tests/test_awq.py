"""AWQ helpers that need no GPU: the plain quantiser's round trip and the config."""
import pytest
import torch

ORDER = [0, 2, 4, 6, 1, 3, 5, 7]


def unpack(words, N):  # int32 [R, N/8] -> [R, N]: nibble i of word j is column 8 j + ORDER[i]
    out = torch.empty(words.shape[0], N, dtype=torch.int64)
    for i, c in enumerate(ORDER):
        out[:, c::8] = (words.to(torch.int64) >> (4 * i)) & 15
    return out


@pytest.mark.parametrize("G", [32, 128])
def test_quantize_awq_round_trip_within_half_a_step(G):
    from light_vllm_amd.quantization import quantize_awq
    w = torch.randn(64, 256, generator=torch.Generator().manual_seed(G)) * 0.05
    qweight, qzeros, scales = quantize_awq(w, G)
    assert qweight.shape == (256, 8) and qzeros.shape == (256 // G, 8) and scales.shape == (256 // G, 64)
    s = scales.double().repeat_interleave(G, 0)
    wd = (unpack(qweight, 64) - unpack(qzeros, 64).repeat_interleave(G, 0)).double() * s  # [K, N]
    assert bool(((w.t().double() - wd).abs() <= s / 2).all())


def test_awq_config():
    from light_vllm_amd.quantization import AWQConfig
    a = AWQConfig.from_config({"w_bit": 4, "q_group_size": 128, "zero_point": True})
    b = AWQConfig.from_config({"bits": 4, "group_size": 64, "zero_point": True})
    assert (a.group_size, b.group_size, a.pack_factor, a.get_name()) == (128, 64, 8, "awq")
    with pytest.raises(ValueError):
        AWQConfig.from_config({"bits": 8, "group_size": 128, "zero_point": True})
