"""static_scaled_int8_quant / dynamic_scaled_int8_quant (csrc/int8_quant.hip) against their arithmetic restated in
fp32 torch on the CPU (IEEE division and multiplication, torch.round = halves to even): q and scale bit-equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
# a wave per row (twice), a workgroup per row; then the two other paths of the kernel: rows that are no multiple of 16
# bytes (scalar loops) and a row longer than the registers hold (16384 elements of 16 bits), re-read in the second pass
SHAPES = [(1, 64), (3, 200), (5, 4096 + 8), (2, 67), (2, 16384 + 8)]


def ref_dynamic(x):
    xf = x.cpu().float()
    a = xf.abs().amax(dim=1, keepdim=True)
    c127 = torch.full_like(a, 127.0)  # tensor operands: an IEEE fp32 division per element
    inv = torch.where(a > 0, c127 / a, torch.zeros_like(a))
    return torch.round(xf * inv).clamp(-128, 127).to(torch.int8), a / c127


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_dynamic_is_bit_equal(ops, dtype, shape):
    x = (torch.randn(*shape, generator=torch.Generator().manual_seed(shape[1])) * 3).to(dtype).to(DEV)
    q, s = ops.scaled_int8_quant(x)
    rq, rs = ref_dynamic(x)
    assert s.shape == (shape[0], 1) and s.dtype == torch.float32
    assert torch.equal(s.cpu(), rs) and torch.equal(q.cpu(), rq)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dynamic_ties_outlier_and_zero_rows(ops, dtype):
    x = torch.zeros(3, 200)
    x[0, :7] = torch.tensor([127.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5])  # scale exactly 1: every half is a tie
    x[1] = 1e-3
    x[1, 77] = -3e4  # one huge value, the rest tiny
    q, s = ops.scaled_int8_quant(x.to(dtype).to(DEV))
    rq, rs = ref_dynamic(x.to(dtype))
    assert torch.equal(s.cpu(), rs) and torch.equal(q.cpu(), rq)
    assert q[0, :7].tolist() == [127, 0, 0, 2, -2, 2, -2] and s[0].item() == 1.0
    assert q[1, 77].item() == -127 and q[1].count_nonzero().item() == 1
    assert s[2].item() == 0.0 and q[2].count_nonzero().item() == 0  # all-zero row: scale 0 and zeros, no NaN


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_static_is_bit_equal_and_saturates(ops, dtype, shape):
    x = (torch.randn(*shape, generator=torch.Generator().manual_seed(shape[1])) * 3).to(dtype)
    x[0, :2] = torch.tensor([100.0, -100.0]).to(dtype)
    scale = torch.tensor([0.05], dtype=torch.float32)
    q, s = ops.scaled_int8_quant(x.to(DEV), scale.to(DEV))
    ref = torch.round(x.float() / scale.expand(shape)).clamp(-128, 127).to(torch.int8)
    assert torch.equal(q.cpu(), ref) and s.item() == scale.item()
    assert q[0, 0].item() == 127 and q[0, 1].item() == -128
