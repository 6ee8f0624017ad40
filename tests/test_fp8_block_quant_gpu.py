"""per_token_group_fp8_quant (csrc/fp8_block_quant.hip) bit for bit against its formula restated in torch fp32 on the
CPU: per group of 128 channels s = max(absmax, 1e-10) / 448, xq = e4m3(clamp(x / s, +-448)), a NaN quotient -> +448,
NaNs skipped by the absmax.  IEEE division and round-to-nearest-even on both sides, so bytes and scales are equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def restated(x):
    M, K = x.shape
    g = x.float().view(M, K // 128, 128)
    s = torch.where(g.isnan(), 0.0, g.abs()).amax(dim=2, keepdim=True).clamp_min(1e-10) / 448.0
    q = g / s
    q = torch.where(q.isnan(), 448.0, q.clamp(-448.0, 448.0))
    return q.to(torch.float8_e4m3fn).view(M, K), s.view(M, K // 128)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,K,strided", [(1, 128, False), (7, 640, False), (64, 14336, False), (7, 640, True)])
def test_per_token_group_fp8_quant_bits(ops, M, K, strided, dtype):
    g = torch.Generator().manual_seed(M + K)
    groups = torch.randn(M * K // 128, 128, generator=g) * 4.0 ** torch.randint(-4, 4, (M * K // 128, 1), generator=g)
    if len(groups) > 3:
        groups[1] = 0                                              # all zero: scale 1e-10 / 448, zeros out
        groups[2] = groups[2].clamp(-50, 50)
        groups[2, 5] = -448 * 2.0 ** -3                            # max exactly 448 * 2^j: scale 2^j, the element -448
        groups[3, 7], groups[3, 9] = float("inf"), float("nan")    # scale inf: finite -> 0, inf / inf and NaN -> +448
    x = groups.view(M, K).to(dtype)
    xd = x.to(DEV)
    if strided:  # a column slice of a wider tensor: row stride K + 256 elements
        wide = torch.zeros(M, K + 256, dtype=dtype, device=DEV)
        wide[:, 128:128 + K] = xd
        xd = wide[:, 128:128 + K]
    xq, xs = torch.ops._C_amd.per_token_group_fp8_quant(xd)
    rq, rs = restated(x)
    assert xq.dtype == torch.float8_e4m3fn and xq.shape == (M, K) and xs.shape == (M, K // 128)
    assert torch.equal(xs.cpu(), rs)
    assert torch.equal(xq.cpu().view(torch.uint8), rq.view(torch.uint8))
    if len(groups) > 3:
        flat_s, flat_q = rs.view(-1), rq.view(-1, 128).float()
        assert flat_s[1] == torch.tensor(1e-10) / 448 and (flat_q[1] == 0).all()
        assert flat_s[2] == 2.0 ** -3 and flat_q[2, 5] == -448 and flat_s[3] == float("inf") and flat_q[3, 9] == 448
