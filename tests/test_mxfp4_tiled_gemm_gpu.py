"""LDS-tiled W4A8 MXFP4 GEMM (csrc/mxfp4_tiled_gemm.hip) against float64 on the CPU from the same code and scale bytes;
the operands, the exact grid and the ulp are test_mxfp4_gemm_gpu.py's.  A workgroup tile is 128 rows x 128 columns (2 x
2 waves of 64 x 64), a chunk is one k-step of 128 k, a loop trip is one scale word of 4 k-steps, and K is split in
whole scale words (at least 2 per split, at most 16 splits) when the tiles do not fill the device."""
import ctypes

import pytest
import torch

from test_mxfp4_gemm_gpu import DEV, operands, ulp

pytestmark = pytest.mark.gpu
HUGE = 1 << 30


def tiled(xq, wp, ep, sx, N, K, dtype, bias=None):
    return torch.ops._C_amd.linear_w4a8_mxfp4_tiled(xq, wp, ep, sx.to(DEV), N, K,
                                                    None if bias is None else bias.to(DEV), dtype)


def packed(codes, scales):
    return torch.ops._C_amd.mxfp4_pack(codes.to(DEV), scales.to(DEV))


SHAPES = [(1, 16, 128),      # one row, one n-tile, one step: three dead bytes in the scale word
          (129, 144, 640),   # a second workgroup row with one live row, a second workgroup column with one live
                             # n-tile, 5 steps: the second scale word has one live byte
          (200, 272, 1536),  # the wave boundary at 64 rows inside the second m-block, 17 n-tiles, three whole scale
                             # words and no split (a split owns at least two)
          (65, 32, 4224),    # 33 steps = 9 scale words over 3 K splits, the last word with one live step
          (70, 48, 14336)]   # 28 words in 14 splits of two, the 1024-k floor: the reduce kernel sums many slabs


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("scaled", [False, True], ids=["pow2", "per_token_bias"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_tiled_gemm_on_the_exact_grid(ops, M, N, K, scaled, dtype):
    xq, codes, scales, acc, _ = operands(M, N, K)
    g = torch.Generator().manual_seed(N)
    sx = (torch.rand(M, generator=g) + 0.5) * 1e-2 if scaled else torch.tensor([2.0 ** -5])
    bias = (torch.randn(N, generator=g) * 0.5).to(dtype) if scaled else None
    y = tiled(xq.to(DEV), *packed(codes, scales), sx, N, K, dtype, bias).cpu()
    ref = acc * sx.double().reshape(-1, 1) + (0 if bias is None else bias.double())
    assert y.shape == (M, N) and y.dtype == dtype
    if not scaled:
        assert torch.equal(y, ref.to(dtype))
    else:
        err = (y.double() - ref).abs() / ulp(ref, dtype)
        assert (err <= 1).all(), err.max().item()


def test_wide_code_range(ops):
    M, N, K = 129, 144, 4224
    xq, codes, scales, acc, mag = operands(M, N, K, True)
    g = torch.Generator().manual_seed(1)
    sx = (torch.rand(M, generator=g) + 0.5) * 1e-3 * 4.0 ** torch.randint(-3, 3, (M,), generator=g)
    bias = (torch.randn(N, generator=g) * 0.5).to(torch.bfloat16)
    ref = acc * sx.double().reshape(-1, 1) + bias.double()
    bound = K * 2.0 ** -24 * mag * sx.double().reshape(-1, 1) + ulp(ref, torch.bfloat16)
    err = (tiled(xq.to(DEV), *packed(codes, scales), sx, N, K, torch.bfloat16, bias).cpu().double() - ref).abs()
    print("worst error / bound:", (err / bound).max().item())
    assert (err <= bound).all(), (err / bound).max().item()


def test_routing_by_mxfp4_tiled_min_rows(ops):
    M, N, K = 150, 48, 640
    xq, codes, scales, _, _ = operands(M, N, 3 * K, True)
    wp, ep = packed(codes[:, K // 2:K].contiguous(), scales[:, K // 32:2 * K // 32].contiguous())
    x = xq.to(DEV)[:, K:2 * K]  # a column slice: row stride 3 K bytes
    sx = (torch.rand(M, generator=torch.Generator().manual_seed(2)) + 0.5).to(DEV)
    op = lambda x_, s_: torch.ops._C_amd.skinny_linear_w4a8_mxfp4(x_, wp, ep, s_, N, K, None, torch.bfloat16)  # noqa: E731
    get, put = torch.ops._C_amd.get_tuning, torch.ops._C_amd.set_tuning
    rows = get("mxfp4_tiled_min_rows")
    try:
        put("mxfp4_tiled_min_rows", 65)
        assert torch.equal(op(x, sx), tiled(x, wp, ep, sx, N, K, torch.bfloat16))
        put("mxfp4_tiled_min_rows", HUGE)
        assert torch.equal(op(x, sx), torch.cat([op(x[a:b], sx[a:b]) for a, b in ((0, 64), (64, 128), (128, 150))]))
    finally:
        put("mxfp4_tiled_min_rows", rows)


@pytest.mark.parametrize("M,K,rc", [(8, 128, 0), (300, 128, 0), (8, 192, 3)])
def test_c_entry(ops, M, K, rc):
    from light_vllm_amd import _native
    lib = _native.load_hip_library()
    lib.lvllm_gemm_w4a8_mxfp4.restype = ctypes.c_int
    lib.lvllm_gemm_w4a8_mxfp4_workspace_bytes.restype = ctypes.c_int64
    N = 16
    xq, codes, scales, acc, _ = operands(M, N, 128)
    wp, ep = packed(codes, scales)
    x, sx = xq.to(DEV), torch.ones(M, device=DEV)
    y = torch.full((M, N), 7.0, dtype=torch.float16, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    got = lib.lvllm_gemm_w4a8_mxfp4(p(y), p(x), p(wp), p(ep), p(sx), None, M, N, K, ctypes.c_int64(K), 1, None,
                                    ctypes.c_int64(0), None)
    torch.cuda.synchronize()
    assert got == rc
    if rc == 0:
        assert torch.equal(y.cpu(), acc.to(torch.float16))
    else:  # refused: an error code, the text, and nothing launched
        assert b"envelope" in lib.lvllm_last_error() and (y == 7.0).all()
    # a workspace exactly when the plan splits K: one tile of 1024 k cannot (a split owns 1024 k), 4096 k does
    ws = lib.lvllm_gemm_w4a8_mxfp4_workspace_bytes
    assert ws(M, N, 128) == 0 and ws(M, N, 1024) == 0 and ws(M, N, 4096) == 4 * M * N * 4 and ws(M, N, 192) == 0
