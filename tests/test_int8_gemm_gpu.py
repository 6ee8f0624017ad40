"""W8A8 int8 weight-streaming GEMM (csrc/int8_gemm.hip): acc = Xq . Wq^T is an int32, so the result without bias must
EQUAL T(sx[m] * (sw[n] * float(acc))) formed in fp32 in that order; with bias the kernel adds in fp32 and may or may
not fuse the add, which is one unit in the last place of T against the sum formed in float64."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]


def operands(M, N, K, seed):
    """Xq, Wq over all of [-128, 127]; positive scales of mixed magnitude."""
    g = torch.Generator().manual_seed(seed)
    xq = torch.randint(-128, 128, (M, K), generator=g, dtype=torch.int8)
    wq = torch.randint(-128, 128, (N, K), generator=g, dtype=torch.int8)
    sx = (torch.rand(M, generator=g) + 0.5) * 1e-2 * 4.0 ** torch.randint(-3, 3, (M,), generator=g)
    sw = (torch.rand(N, generator=g) + 0.5) * 1e-3 * 4.0 ** torch.randint(-3, 3, (N,), generator=g)
    return xq, wq, sx, sw


def reference(xq, wq, sx, sw):
    acc = xq.long() @ wq.long().t()
    return sx[:, None] * (sw[None, :] * acc.float())  # fp32, the weight scale first


def run(xq, wq, sx, sw, dtype, bias=None):
    N, K = wq.shape
    return torch.ops._C_amd.skinny_linear_w8a8_int8(xq.to(DEV), torch.ops._C_amd.int8_pack(wq.to(DEV)), sx.to(DEV),
                                                    sw.to(DEV), N, K, None if bias is None else bias.to(DEV), dtype).cpu()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("use_bias", [False, True])
@pytest.mark.parametrize("M,N,K,wgs", [(1, 16, 64, 0), (5, 48, 192, 0), (17, 64, 448, 0), (33, 32, 8256, 0),
                                       (64, 272, 1024, 0), (64, 272, 1024, 9),
                                       # waves own up to 4 k-steps above (or K is split); 5..8 steps per wave take the
                                       # 8-step variant within ONE workgroup, with one m-tile
                                       (1, 48, 4096, 0),
                                       # 65 k-steps: one past 8 waves x 8 steps, K split in two, four m-tiles
                                       (50, 32, 4160, 0)])
def test_int8_gemm_is_exact(ops, dtype, use_bias, M, N, K, wgs):
    xq, wq, sx, sw = operands(M, N, K, M + N + K)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(N)) * 0.5).to(dtype) if use_bias else None
    default = torch.ops._C_amd.get_tuning("gemm_workgroups")
    try:
        if wgs:
            torch.ops._C_amd.set_tuning("gemm_workgroups", wgs)
        y = run(xq, wq, sx, sw, dtype, bias)
    finally:
        torch.ops._C_amd.set_tuning("gemm_workgroups", default)
    ref = reference(xq, wq, sx, sw)
    assert y.shape == (M, N) and y.dtype == dtype
    if not use_bias:
        assert torch.equal(y, ref.to(dtype))
        return
    ref64 = ref.double() + bias.double()
    mant, min_exp = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    ulp = 2.0 ** (torch.floor(torch.log2(ref64.abs().clamp_min(2.0 ** min_exp))) - mant)
    assert ((y.double() - ref64).abs() <= ulp).all(), ((y.double() - ref64).abs() / ulp).max().item()


def test_cancellation_needs_integer_partials(ops):
    """Every wave's and workgroup's partial sum is far beyond 2^24 while the total is 16129 * 2 (m + 1): any partial
    that travelled as fp32 would lose the low bits."""
    M, N, K = 16, 16, 8256
    wq = torch.full((N, K), 127, dtype=torch.int8)
    xq = torch.full((M, K), 127, dtype=torch.int8)
    xq[:, K // 2:] = -127
    for m in range(M):
        xq[m, K - (m + 1):] = 127
    sx, sw = torch.ones(M), torch.full((N,), 2.0 ** -6)
    ref = reference(xq, wq, sx, sw)
    assert torch.equal(ref[:, 0], torch.arange(1, M + 1) * (16129 * 2 / 64))
    assert torch.equal(run(xq, wq, sx, sw, torch.float16), ref.to(torch.float16))


def test_strided_rows_and_100_rows(ops):
    N, K = 64, 512
    xq, wq, sx, sw = operands(100, N, 3 * K, 3)
    wq = wq[:, :K].contiguous()
    wp = torch.ops._C_amd.int8_pack(wq.to(DEV))
    op = lambda x, s: torch.ops._C_amd.skinny_linear_w8a8_int8(x, wp, s.to(DEV), sw.to(DEV), N, K, None, torch.bfloat16).cpu()  # noqa: E731
    big = xq.to(DEV)
    x = big[:, K:2 * K]  # a column slice: row stride 1536 bytes
    assert torch.equal(op(x[:8], sx[:8]), reference(xq[:8, K:2 * K], wq, sx[:8], sw).to(torch.bfloat16))
    # above 64 rows: chunks of 64 through the same kernel, equal row for row to the <= 64 path
    y = op(x, sx)
    assert torch.equal(y, torch.cat([op(x[:64].contiguous(), sx[:64]), op(x[64:].contiguous(), sx[64:])]))
    assert torch.equal(y, reference(xq[:, K:2 * K], wq, sx, sw).to(torch.bfloat16))


def test_cutlass_scaled_mm(ops):
    dtype = torch.float16
    xq, wq, sx, sw = operands(7, 48, 256, 11)
    b = wq.to(DEV).t()  # [K, N], strides (1, K), as the reference passes weight.t()
    y = ops.cutlass_scaled_mm(xq.to(DEV), b, sx.to(DEV).reshape(-1, 1), sw.to(DEV).reshape(-1, 1), dtype)
    assert torch.equal(y.cpu(), run(xq, wq, sx, sw, dtype))
    one = sx[:1]  # a scalar scale equals its expansion
    assert torch.equal(ops.cutlass_scaled_mm(xq.to(DEV), b, one.to(DEV), sw.to(DEV), dtype).cpu(),
                       run(xq, wq, one.expand(7).contiguous(), sw, dtype))
    # K % 64 != 0 and N % 16 != 0: the exact fallback, same epilogue
    xq, wq, sx, sw = operands(7, 24, 96, 12)
    y = ops.cutlass_scaled_mm(xq.to(DEV), wq.to(DEV).t(), sx.to(DEV), sw.to(DEV), dtype)
    assert torch.equal(y.cpu(), reference(xq, wq, sx, sw).to(dtype))
    with pytest.raises(RuntimeError, match="int8"):
        ops.cutlass_scaled_mm(xq.to(DEV).half(), wq.to(DEV).t().half(), sx.to(DEV), sw.to(DEV), dtype)


@pytest.mark.parametrize("M,K", [(65, 128), (8, 96)])
def test_c_entry_returns_3_outside_the_envelope(ops, M, K):
    from light_vllm_amd import _native
    lib = _native.load_hip_library()
    lib.lvllm_skinny_gemm_w8a8_int8.restype = ctypes.c_int
    N = 16
    x = torch.zeros(M, K, dtype=torch.int8, device=DEV)
    w = torch.zeros(N, K, dtype=torch.int8, device=DEV)
    sx, sw = torch.ones(M, device=DEV), torch.ones(N, device=DEV)
    y = torch.empty(M, N, dtype=torch.float16, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.lvllm_skinny_gemm_w8a8_int8(p(y), p(x), p(w), p(sx), p(sw), None, M, N, K, ctypes.c_int64(K), 1, None,
                                         ctypes.c_int64(0), None)
    assert rc == 3
