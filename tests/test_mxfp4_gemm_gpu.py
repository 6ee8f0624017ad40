"""W4A8 MXFP4 decode GEMM (csrc/mxfp4_gemm.hip) against float64 on the CPU from the same code and scale bytes, through
a 16-entry table: ref = sx * sum_k x w4 2^(e - 127) (+ bias).  On the exact grid every fp32 partial sum is exact in any
order, so the test demands equality: that fixes which nibble is the lower k, the lane <-> k map of both operands, the
op_sel byte and which lane's scale byte the matrix pipe applies.  Over the full code range the bound is that of a
K-term fp32 sum, as in test_fp8_tiled_gemm_gpu.py."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F8 = torch.float8_e4m3fn
E2M1 = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6], dtype=torch.float64)


def weight(codes, scales):
    """float64 [N, K] from the checkpoint bytes: even k in the low nibble, one scale per 32 k"""
    w = E2M1[torch.stack((codes & 15, codes >> 4), dim=2).reshape(codes.shape[0], -1).long()]
    return w * torch.exp2(scales.double() - 127).repeat_interleave(32, dim=1)


@functools.lru_cache(maxsize=None)
def operands(M, N, K, wide=False):
    """(xq fp8, codes [N, K/2], scales [N, K/32]) on the CPU, the float64 product and sum_k |x||w| 2^(e - 127).  Weight
    codes are uniform over all 16.  Exact grid: x multiples of 1/8 in [-1.875, 1.875], scale codes 125 .. 128, so every
    product is a multiple of 2^-4 2^-2 and every partial sum exact in fp32 (checked below).  Wide: every finite e4m3fn
    code, scale codes 115 .. 139 drawn per block."""
    g = torch.Generator().manual_seed(M + N + K)
    codes = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    if wide:
        finite = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=torch.uint8)
        xq = finite[torch.randint(0, 254, (M, K), generator=g)].view(F8)
        scales = torch.randint(115, 140, (N, K // 32), generator=g, dtype=torch.uint8)
    else:
        xq = (torch.randint(-15, 16, (M, K), generator=g).float() / 8).to(F8)
        scales = torch.randint(125, 129, (N, K // 32), generator=g, dtype=torch.uint8)
    x, w = xq.double(), weight(codes, scales)
    acc, mag = x @ w.t(), x.abs() @ w.abs().t()
    assert wide or mag.max().item() / 2.0 ** -6 < 2 ** 24
    return xq, codes, scales, acc, mag


def ulp(ref, dtype):
    mant, min_exp = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    return 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** min_exp))) - mant)


def run(xq, codes, scales, sx, dtype, bias=None):
    N, K = codes.shape[0], codes.shape[1] * 2
    wp, ep = torch.ops._C_amd.mxfp4_pack(codes.to(DEV), scales.to(DEV))
    return torch.ops._C_amd.skinny_linear_w4a8_mxfp4(xq.to(DEV), wp, ep, sx.to(DEV), N, K,
                                                     None if bias is None else bias.to(DEV), dtype).cpu()


def check_exact_grid(M, N, K, scaled, dtype):
    xq, codes, scales, acc, _ = operands(M, N, K)
    g = torch.Generator().manual_seed(N)
    sx = (torch.rand(M, generator=g) + 0.5) * 1e-2 if scaled else torch.tensor([2.0 ** -5])
    bias = (torch.randn(N, generator=g) * 0.5).to(dtype) if scaled else None
    y = run(xq, codes, scales, sx, dtype, bias)
    ref = acc * sx.double().reshape(-1, 1) + (0 if bias is None else bias.double())
    assert y.shape == (M, N) and y.dtype == dtype
    if not scaled:
        assert torch.equal(y, ref.to(dtype))
    else:
        err = (y.double() - ref).abs() / ulp(ref, dtype)
        assert (err <= 1).all(), err.max().item()


# A k-step is 128 k; a wave owns 1 step up to K = 1024, 2 up to 2048, 4 above; 8 waves x 4 steps = 4096 k per
# workgroup, beyond that K is split over workgroups.  Above 64 rows the op runs chunks of 64 rows.
SHAPES = [(1, 16, 128),      # one step: seven idle waves
          (17, 48, 640),     # m-tile edge (MT = 2); 5 steps, one per wave: scale-word shifts 8, 16, 24, and a second
                             # scale word with one live byte
          (5, 16, 1536),     # 2 steps per wave: the shift by 16, op_sel 0 and 1
          (64, 144, 4096),   # MT = 4, 4 steps per wave, the full workgroup K
          (33, 32, 4224),    # K one step past a workgroup: 2 splits, the second with one live wave
          (3, 16, 14336),    # 4 splits, the last half full
          (65, 32, 512),     # chunks of 64 rows: 64 + 1
          (150, 48, 640)]    # 64 + 64 + 22


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("scaled", [False, True], ids=["pow2", "per_token_bias"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_mxfp4_gemm_on_the_exact_grid(ops, M, N, K, scaled, dtype):
    check_exact_grid(M, N, K, scaled, dtype)


@pytest.mark.parametrize("M,N,K", [(3, 304, 640),     # MT = 1: 19 n-tiles on 7 workgroups, 3 or 2 each: the slot is
                                                      # refilled, a wave meeting per tile
                                   (64, 2304, 256)])  # MT = 4: 18 tiles per workgroup, the 16-tile output stage flushes
def test_many_tiles_per_workgroup(ops, M, N, K):
    get, put = torch.ops._C_amd.get_tuning, torch.ops._C_amd.set_tuning
    groups = get("gemm_workgroups")
    try:
        put("gemm_workgroups", 8)  # the fewest the library takes
        check_exact_grid(M, N, K, False, torch.bfloat16)
    finally:
        put("gemm_workgroups", groups)


def test_wide_code_range(ops):
    M, N, K = 33, 32, 4224
    xq, codes, scales, acc, mag = operands(M, N, K, True)
    g = torch.Generator().manual_seed(1)
    sx = (torch.rand(M, generator=g) + 0.5) * 1e-3 * 4.0 ** torch.randint(-3, 3, (M,), generator=g)
    bias = (torch.randn(N, generator=g) * 0.5).to(torch.bfloat16)
    ref = acc * sx.double().reshape(-1, 1) + bias.double()
    bound = K * 2.0 ** -24 * mag * sx.double().reshape(-1, 1) + ulp(ref, torch.bfloat16)
    err = (run(xq, codes, scales, sx, torch.bfloat16, bias).double() - ref).abs()
    print("worst error / bound:", (err / bound).max().item())
    assert (err <= bound).all(), (err / bound).max().item()


def test_strided_rows(ops):
    M, N, K = 8, 32, 512
    xq, codes, scales, _, _ = operands(M, N, 3 * K)
    codes, scales = codes[:, K // 2:K].contiguous(), scales[:, K // 32:2 * K // 32].contiguous()
    x = xq.to(DEV)[:, K:2 * K]  # a column slice: row stride 1536 bytes
    ref = xq[:, K:2 * K].double() @ weight(codes, scales).t()
    assert torch.equal(run(x, codes, scales, torch.ones(1), torch.bfloat16), ref.to(torch.bfloat16))


def test_pack_is_a_permutation_and_refuses_nan_scales(ops):
    N, K = 48, 640  # 5 k-steps: the second scale word of a lane has one live byte
    g = torch.Generator().manual_seed(0)
    codes = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    scales = torch.randint(0, 255, (N, K // 32), generator=g, dtype=torch.uint8)
    wp, ep = (t.cpu() for t in torch.ops._C_amd.mxfp4_pack(codes.to(DEV), scales.to(DEV)))
    # [tile][step][g][c][16 bytes] = codes[16 tile + c][64 step + 16 g ..]
    assert torch.equal(wp.view(N // 16, K // 128, 4, 16, 16),
                       codes.view(N // 16, 16, K // 128, 4, 16).permute(0, 2, 3, 1, 4))
    # [tile][word][g][c][byte] = scales[16 tile + c][4 (4 word + byte) + g], 127 past K
    padded = torch.full((N, 2 * 16), 127, dtype=torch.uint8)
    padded[:, :K // 32] = scales
    assert torch.equal(ep.view(N // 16, 2, 4, 16, 4), padded.view(N // 16, 16, 2, 4, 4).permute(0, 2, 4, 1, 3))
    scales[3, 7] = 255
    with pytest.raises(RuntimeError, match="0xFF"):
        torch.ops._C_amd.mxfp4_pack(codes.to(DEV), scales.to(DEV))


@pytest.mark.parametrize("M,K,rc", [(8, 128, 0), (65, 128, 3), (8, 192, 3)])
def test_c_entry(ops, M, K, rc):
    from light_vllm_amd import _native
    lib = _native.load_hip_library()
    lib.lvllm_skinny_gemm_w4a8_mxfp4.restype = ctypes.c_int
    lib.lvllm_last_error.restype = ctypes.c_char_p
    N = 16
    xq, codes, scales, acc, _ = operands(M, N, 128)
    wp, ep = torch.ops._C_amd.mxfp4_pack(codes.to(DEV), scales.to(DEV))
    x = xq.to(DEV)
    sx = torch.ones(M, device=DEV)
    y = torch.full((M, N), 7.0, dtype=torch.float16, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    got = lib.lvllm_skinny_gemm_w4a8_mxfp4(p(y), p(x), p(wp), p(ep), p(sx), None, M, N, K, ctypes.c_int64(K), 1, None,
                                           ctypes.c_int64(0), None)
    torch.cuda.synchronize()
    assert got == rc
    if rc == 0:
        assert torch.equal(y.cpu(), acc.to(torch.float16))
    else:  # refused: an error code, the text, and nothing launched
        assert b"envelope" in lib.lvllm_last_error() and (y == 7.0).all()
