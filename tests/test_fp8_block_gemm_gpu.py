"""Block-scaled W8A8 fp8 decode GEMM (csrc/fp8_block_gemm.hip) against float64 on the CPU from the same bytes:
ref = sum_b xs[m, b] ws[n // 128, b] sum_{k in b} xq[m, k] wq[n, k] (+ bias).  On the exact grid (operands multiples of
1/8, power-of-two scales) every fp32 partial sum is exact in any order, so equality is demanded: that fixes the
lane <-> k map of both operands, the two 64-k halves, which block's scale meets which step, the n // 128 row of ws and
the wave and split ownership.  Over the full code range the bound is that of a K-term fp32 sum plus three roundings per
block (the scale product, its product with the partial, the add)."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F8 = torch.float8_e4m3fn


@functools.lru_cache(maxsize=None)
def operands(M, N, K, wide=False):
    """(xq, wq fp8, xs [M, K/128], ws [ceil(N/128), K/128] fp32) on the CPU.  Exact grid: multiples of 1/8 within
    +-1.875, scales 2^-1 or 2^0 per block: every product is a multiple of 2^-6 2^-2, and the sum of their magnitudes
    stays below 2^24 of those (asserted).  Wide: every finite e4m3fn code, scales over six binades."""
    g = torch.Generator().manual_seed(M + N + K)
    B, NB = K // 128, (N + 127) // 128
    if wide:
        finite = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=torch.uint8)
        xq, wq = (finite[torch.randint(0, 254, s, generator=g)].view(F8) for s in ((M, K), (N, K)))
        xs, ws = ((torch.rand(s, generator=g) + 0.5) * 1e-2 * 4.0 ** torch.randint(-3, 3, s, generator=g)
                  for s in ((M, B), (NB, B)))
    else:
        xq, wq = ((torch.randint(-15, 16, s, generator=g).float() / 8).to(F8) for s in ((M, K), (N, K)))
        xs, ws = (2.0 ** torch.randint(-1, 1, s, generator=g) for s in ((M, B), (NB, B)))
        assert reference(xq, wq, xs, ws)[1].max().item() / 2.0 ** -8 < 2 ** 24
    return xq, wq, xs, ws


def reference(xq, wq, xs, ws):
    """float64 product and sum_k |x||w| xs ws"""
    N = wq.shape[0]
    x = xq.double() * xs.double().repeat_interleave(128, dim=1)
    w = wq.double() * ws.double().repeat_interleave(128, dim=0)[:N].repeat_interleave(128, dim=1)
    return x @ w.t(), x.abs() @ w.abs().t()


def ulp(ref, dtype):
    mant, min_exp = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    return 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** min_exp))) - mant)


def run(xq, wq, xs, ws, dtype, bias=None):
    N, K = wq.shape
    wp = torch.ops._C_amd.fp8_block_pack(wq.to(DEV))
    return torch.ops._C_amd.skinny_linear_w8a8_fp8_block(xq.to(DEV), wp, xs.to(DEV), ws.to(DEV), N, K,
                                                         None if bias is None else bias.to(DEV), dtype).cpu()


def check_exact_grid(M, N, K, scaled, dtype):
    xq, wq, xs, ws = operands(M, N, K)
    bias = None
    if scaled:
        # a per-token factor that is no power of two, and a bias.  Each block now costs three fp32 roundings (scale
        # product, its product with the exact partial, the add), the waves and splits one each: at most 3 K / 128 + 40
        # < 400 roundings of 2^-24 relative to sum |terms|.  One ulp of T leaves half an ulp, >= 2^-13 |ref|, for them,
        # which holds when nothing cancels: this case takes the operands' magnitudes and a positive bias, so that
        # |ref| >= sum |terms| and 400 * 2^-24 < 2^-13.  "signed" keeps the signs and demands the same count of
        # roundings as a bound instead: ulp_T(ref) + (3 K / 128 + 40) 2^-24 sum |terms|
        g = torch.Generator().manual_seed(N)
        if scaled == "magnitudes":
            xq, wq = xq.float().abs().to(F8), wq.float().abs().to(F8)
        xs = xs * ((torch.rand(M, 1, generator=g) + 0.5) * 1e-2)
        bias = (torch.randn(N, generator=g) * 0.5).to(dtype)
        bias = bias.abs() if scaled == "magnitudes" else bias
    y = run(xq, wq, xs, ws, dtype, bias)
    acc, mag = reference(xq, wq, xs, ws)
    ref = acc + (0 if bias is None else bias.double())
    assert y.shape == (M, N) and y.dtype == dtype
    if not scaled:
        assert torch.equal(y, ref.to(dtype))
    else:
        slack = (3 * K // 128 + 40) * 2.0 ** -24 * (mag + bias.double().abs()) if scaled == "signed" else 0
        err = (y.double() - ref).abs() / (ulp(ref, dtype) + slack)
        assert (err <= 1).all(), err.max().item()


# A k-step is 128 k = one scale block; a wave owns 1 step up to K = 1024, 2 up to 2048, 4 above; 8 waves x 4 steps =
# 4096 k per workgroup, beyond that K is split over workgroups.  Above 64 rows the op runs chunks of 64 rows.
SHAPES = [(1, 16, 128),      # one step: seven idle waves
          (17, 144, 640),    # m-tile edge (MT = 2); N crosses a scale row at 128 with a 16-row remainder; 5 live waves
          (5, 16, 1536),     # 2 steps per wave
          (64, 272, 4096),   # MT = 4, 4 steps per wave, the full workgroup K; three scale rows
          (33, 32, 4224),    # K one step past a workgroup: 2 splits, the second with one live wave
          (3, 16, 14336),    # 4 splits, the last half full
          (65, 32, 512),     # chunks of 64 rows: 64 + 1
          (150, 48, 640)]    # 64 + 64 + 22


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("scaled", [False, "magnitudes", "signed"], ids=["pow2", "per_token_bias", "signed_bias"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_fp8_block_gemm_on_the_exact_grid(ops, M, N, K, scaled, dtype):
    check_exact_grid(M, N, K, scaled, dtype)


@pytest.mark.parametrize("M,N,K", [(3, 304, 640),     # MT = 1: 19 n-tiles on 7 workgroups, 3 or 2 each: the slot is
                                                      # refilled, a wave meeting per tile
                                   (64, 2304, 256)])  # MT = 4: 18 tiles per workgroup, the output stage flushes
def test_many_tiles_per_workgroup(ops, M, N, K):
    get, put = torch.ops._C_amd.get_tuning, torch.ops._C_amd.set_tuning
    groups = get("gemm_workgroups")
    try:
        put("gemm_workgroups", 8)  # the fewest the library takes
        check_exact_grid(M, N, K, False, torch.bfloat16)
    finally:
        put("gemm_workgroups", groups)


def test_wide_code_range(ops):
    M, N, K = 33, 160, 4224
    xq, wq, xs, ws = operands(M, N, K, True)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(1)) * 0.5).to(torch.bfloat16)
    acc, mag = reference(xq, wq, xs, ws)
    ref = acc + bias.double()
    bound = (K + 3 * K // 128) * 2.0 ** -24 * mag + ulp(ref, torch.bfloat16)
    err = (run(xq, wq, xs, ws, torch.bfloat16, bias).double() - ref).abs()
    print("worst error / bound:", (err / bound).max().item())
    assert (err <= bound).all(), (err / bound).max().item()


def test_strided_rows(ops):
    M, N, K = 8, 32, 512
    xq, wq, xs, ws = operands(M, N, 3 * K)
    wq, xs, ws = wq[:, K:2 * K].contiguous(), xs[:, 4:8].contiguous(), ws[:, 4:8].contiguous()
    x = xq.to(DEV)[:, K:2 * K]  # a column slice: row stride 1536 bytes
    ref = reference(xq[:, K:2 * K], wq, xs, ws)[0]
    assert torch.equal(run(x, wq, xs, ws, torch.bfloat16), ref.to(torch.bfloat16))


def test_pack_is_the_stated_permutation(ops):
    N, K = 48, 640
    wq = torch.randint(0, 256, (N, K), generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    wp = torch.ops._C_amd.fp8_block_pack(wq.to(DEV)).cpu()
    # [tile][step][g][c][half][16 bytes] = wq[16 tile + c][128 step + 64 half + 16 g ..]
    assert torch.equal(wp.view(N // 16, K // 128, 4, 16, 2, 16),
                       wq.view(N // 16, 16, K // 128, 2, 4, 16).permute(0, 2, 4, 1, 3, 5))


@pytest.mark.parametrize("M,K,rc", [(8, 128, 0), (65, 128, 3), (8, 192, 3)])
def test_c_entry(ops, M, K, rc):
    from light_vllm_amd import _native
    lib = _native.load_hip_library()
    lib.lvllm_skinny_gemm_w8a8_fp8_block.restype = ctypes.c_int
    lib.lvllm_last_error.restype = ctypes.c_char_p
    N = 16
    xq, wq, xs, ws = operands(M, N, 128)
    wp = torch.ops._C_amd.fp8_block_pack(wq.to(DEV))
    x, sx, sw = xq.to(DEV), xs.to(DEV), ws.to(DEV)
    y = torch.full((M, N), 7.0, dtype=torch.float16, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    got = lib.lvllm_skinny_gemm_w8a8_fp8_block(p(y), p(x), p(wp), p(sx), p(sw), None, M, N, K, ctypes.c_int64(K), 1,
                                               None, ctypes.c_int64(0), None)
    torch.cuda.synchronize()
    assert got == rc
    if rc == 0:
        assert torch.equal(y.cpu(), reference(xq, wq, xs, ws)[0].to(torch.float16))
    else:  # refused: an error code, the text, and nothing launched
        assert b"envelope" in lib.lvllm_last_error() and (y == 7.0).all()
