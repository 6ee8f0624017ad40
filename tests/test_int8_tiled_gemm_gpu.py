"""LDS-tiled W8A8 int8 GEMM (csrc/int8_tiled_gemm.hip): acc = Xq . Wq^T is an int32 however K is chunked or split, so
without bias the result must EQUAL T(sx[m] * (sw[n] * float(acc))) formed in fp32 in that order; with bias the kernel
adds in fp32, one unit in the last place of T against the sum formed in float64."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HUGE = 1 << 30


@functools.lru_cache(maxsize=None)
def operands(M, N, K):
    """Xq, Wq over all of [-128, 127]; positive scales of mixed magnitude; the fp32 reference (weight scale first)."""
    g = torch.Generator().manual_seed(M + N + K)
    xq = torch.randint(-128, 128, (M, K), generator=g, dtype=torch.int8)
    wq = torch.randint(-128, 128, (N, K), generator=g, dtype=torch.int8)
    sx = (torch.rand(M, generator=g) + 0.5) * 1e-2 * 4.0 ** torch.randint(-3, 3, (M,), generator=g)
    sw = (torch.rand(N, generator=g) + 0.5) * 1e-3 * 4.0 ** torch.randint(-3, 3, (N,), generator=g)
    return xq, wq, sx, sw, reference(xq, wq, sx, sw)


def reference(xq, wq, sx, sw):
    return sx[:, None] * (sw[None, :] * (xq.long() @ wq.long().t()).float())


def tiled(xq, wq, sx, sw, dtype, bias=None):
    N, K = wq.shape
    return torch.ops._C_amd.linear_w8a8_int8_tiled(xq.to(DEV), torch.ops._C_amd.int8_pack(wq.to(DEV)), sx.to(DEV),
                                                   sw.to(DEV), N, K, None if bias is None else bias.to(DEV), dtype).cpu()


# The workgroup tile is 128 rows x 128 columns, a K-chunk two k-steps of 64, LDS holds two chunks.
SHAPES = [(1, 16, 64),        # M = 1; N = 16: one n-tile, narrower than a wave's 64 columns; K = 64: half a chunk
          (37, 48, 192),      # M no multiple of 16; one chunk and a half
          (129, 144, 832),    # one row past a 128-row tile; one n-tile past a 128-column tile; 6 chunks + one k-step
          (200, 272, 1088),   # 2 x 3 workgroup tiles, 8 chunks + one k-step
          (130, 32, 8256)]    # 2 tiles on 256 CUs: K split 8 ways, 9 chunks each, the last split one and a half


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("use_bias", [False, True])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_tiled_int8_gemm_is_exact(ops, M, N, K, use_bias, dtype):
    xq, wq, sx, sw, ref = operands(M, N, K)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(N)) * 0.5).to(dtype) if use_bias else None
    y = tiled(xq, wq, sx, sw, dtype, bias)
    assert y.shape == (M, N) and y.dtype == dtype
    if not use_bias:
        assert torch.equal(y, ref.to(dtype))
        return
    ref64 = ref.double() + bias.double()
    mant, min_exp = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    ulp = 2.0 ** (torch.floor(torch.log2(ref64.abs().clamp_min(2.0 ** min_exp))) - mant)
    assert ((y.double() - ref64).abs() <= ulp).all(), ((y.double() - ref64).abs() / ulp).max().item()


def test_split_k_partials_are_integers(ops):
    """One tile, K split 8 ways of 1152 k: seven of the eight partials are beyond 2^24 in magnitude (the one that
    straddles K / 2 largely cancels) while the total is 16129 * 2 (m + 1), so a partial that travelled as fp32 would
    lose the low bits."""
    M, N, K = 16, 16, 8256
    wq = torch.full((N, K), 127, dtype=torch.int8)
    xq = torch.full((M, K), 127, dtype=torch.int8)
    xq[:, K // 2:] = -127
    for m in range(M):
        xq[m, K - (m + 1):] = 127
    sx, sw = torch.ones(M), torch.full((N,), 2.0 ** -6)
    ref = reference(xq, wq, sx, sw)
    assert torch.equal(ref[:, 0], torch.arange(1, M + 1) * (16129 * 2 / 64))
    assert torch.equal(tiled(xq, wq, sx, sw, torch.float16), ref.to(torch.float16))


def test_strided_rows_and_dispatch(ops):
    """150 rows of a column slice (row stride 3 K): the tiled op, the linear at the default threshold and the linear
    with the threshold above M (64-row chunks of the streaming kernel) agree bit for bit."""
    N, K = 64, 512
    xq, wq, sx, sw, _ = operands(150, N, 3 * K)
    wq = wq[:, :K].contiguous()
    wp = torch.ops._C_amd.int8_pack(wq.to(DEV))
    x = xq.to(DEV)[:, K:2 * K]
    args = (x, wp, sx.to(DEV), sw.to(DEV), N, K, None, torch.bfloat16)
    ref = reference(xq[:, K:2 * K], wq, sx, sw).to(torch.bfloat16)
    default = torch.ops._C_amd.get_tuning("int8_tiled_min_rows")
    try:
        y_tiled = torch.ops._C_amd.linear_w8a8_int8_tiled(*args).cpu()
        y_auto = torch.ops._C_amd.skinny_linear_w8a8_int8(*args).cpu()
        torch.ops._C_amd.set_tuning("int8_tiled_min_rows", 65)  # the linear dispatches to the tiled kernel
        y_low = torch.ops._C_amd.skinny_linear_w8a8_int8(*args).cpu()
        torch.ops._C_amd.set_tuning("int8_tiled_min_rows", HUGE)
        y_chunks = torch.ops._C_amd.skinny_linear_w8a8_int8(*args).cpu()
    finally:
        torch.ops._C_amd.set_tuning("int8_tiled_min_rows", default)
    for y in (y_tiled, y_auto, y_low, y_chunks):
        assert torch.equal(y, ref)


@pytest.mark.parametrize("N,K,alloc_k", [(16, 96, 96), (24, 64, 64), (16, 131072, 64)])
def test_c_entry_returns_3_outside_the_envelope(ops, N, K, alloc_k):
    from light_vllm_amd import _native
    lib = _native.load_hip_library()
    lib.lvllm_gemm_w8a8_int8.restype = ctypes.c_int
    M = 8
    x = torch.zeros(M, alloc_k, dtype=torch.int8, device=DEV)
    w = torch.zeros(N, alloc_k, dtype=torch.int8, device=DEV)
    sx, sw = torch.ones(M, device=DEV), torch.ones(N, device=DEV)
    y = torch.full((M, N), 7.0, dtype=torch.float16, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.lvllm_gemm_w8a8_int8(p(y), p(x), p(w), p(sx), p(sw), None, M, N, K, ctypes.c_int64(K), 1, None,
                                  ctypes.c_int64(0), None)
    torch.cuda.synchronize()
    assert rc == 3
    assert (y == 7.0).all()
