"""LDS-tiled W4A16 (AWQ int4) GEMM for prefill batches (csrc/awq_tiled_gemm.hip): the dequantised weight bit for bit
against a torch restatement of the checkpoint semantics, the GEMM against the fp32 matmul of that weight (tolerance of
the kernel family, tests/test_awq_gemm_gpu.py: output rounding + accumulation order; Wd itself is exact)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
ORDER = [0, 2, 4, 6, 1, 3, 5, 7]
HUGE = 1 << 30


def checkpoint(K, N, G, dtype, seed):
    """Random checkpoint tensors (q and z over all of 0..15, positive scales of mixed magnitude), packed, and their Wd."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = torch.randint(0, 16, (K, N), generator=g, device=DEV)
    z = torch.randint(0, 16, (K // G, N), generator=g, device=DEV)
    s = (torch.rand(K // G, N, generator=g, device=DEV) * 0.02 + 1e-3) * 4.0 ** torch.randint(-2, 3, (K // G, N), generator=g, device=DEV)
    s = s.to(dtype)

    def pack(v):  # nibble i of word j = column 8 j + ORDER[i]
        v = v.reshape(v.shape[0], N // 8, 8)
        w = sum(v[:, :, c] << (4 * i) for i, c in enumerate(ORDER))
        return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)

    zr, sr = z.repeat_interleave(G, 0), s.repeat_interleave(G, 0)
    wd = ((q - zr).float() * sr.float()).to(dtype)
    w4, meta = torch.ops._C_amd.awq_pack(pack(q), pack(z), s)
    return w4, meta, wd


def close(y, ref, dtype):
    err, scale = (y.float() - ref).abs().max().item(), ref.abs().max().item()
    return err <= (2 ** -7 if dtype == torch.bfloat16 else 2 ** -9) * scale + 1e-3, (err, scale)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,N,G", [(256, 48, 64), (384, 144, 32)])
def test_every_nibble_is_pinned_bit_for_bit(ops, dtype, K, N, G):
    """x = eye(K): one non-zero product per output, no accumulation error; two / three m-tiles of 128 rows, n past one
    128-column tile, two / four groups per k-block."""
    w4, meta, wd = checkpoint(K, N, G, dtype, K + N)
    x = torch.eye(K, device=DEV, dtype=dtype)
    assert torch.equal(torch.ops._C_amd.linear_w4a16_tiled(x, w4, meta, N, K, G, None), wd)


# The workgroup tile is 128 rows x 128 columns (a wave: 128 x 32), a k-block of 128 is two LDS chunks.
SHAPES = [(1, 16, 128, 128),       # M = 1; one n-tile, narrower than a wave's 32 columns; one k-block
          (65, 48, 384, 64),       # first row count past the decode kernel, no multiple of 16; an odd number of k-blocks
          (129, 144, 640, 32),     # one row past a 128-row tile; one n-tile past a 128-column tile
          (200, 272, 1152, 128),   # 2 x 3 workgroup tiles
          (130, 32, 8320, 128)]    # 2 tiles on 256 CUs, 65 k-blocks: K split 8 ways, 9 k-blocks each, the last split 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("use_bias", [False, True])
@pytest.mark.parametrize("M,N,K,G", SHAPES)
def test_tiled_w4a16_matches_fp32_matmul(ops, dtype, use_bias, M, N, K, G):
    w4, meta, wd = checkpoint(K, N, G, dtype, M + N + K)
    g = torch.Generator(device=DEV).manual_seed(M)
    x = (torch.randn(M, K, generator=g, device=DEV) * 0.5).to(dtype)
    b = (torch.randn(N, generator=g, device=DEV) * 0.5).to(dtype) if use_bias else None
    y = torch.ops._C_amd.linear_w4a16_tiled(x, w4, meta, N, K, G, b)
    ref = x.float() @ wd.float() + (b.float() if use_bias else 0)
    assert y.shape == (M, N) and y.dtype == dtype
    ok, info = close(y, ref, dtype)
    assert ok, info


def test_strided_rows_and_dispatch(ops):
    """150 rows of a column slice (row stride 3 K): the tiled op and the linear routed to the tiled kernel agree bit for
    bit; routed to dequantise + library GEMM the linear is still within tolerance."""
    N, K, G, dtype = 64, 512, 128, torch.bfloat16
    w4, meta, wd = checkpoint(K, N, G, dtype, 1)
    big = (torch.randn(150, 3 * K, generator=torch.Generator(device=DEV).manual_seed(0), device=DEV) * 0.5).to(dtype)
    x = big[:, K:2 * K]
    ref = x.float() @ wd.float()
    lo, hi = torch.ops._C_amd.get_tuning("w4_tiled_min_rows"), torch.ops._C_amd.get_tuning("w4_tiled_max_rows")
    try:
        y_tiled = torch.ops._C_amd.linear_w4a16_tiled(x, w4, meta, N, K, G, None)
        torch.ops._C_amd.set_tuning("w4_tiled_min_rows", 65)
        torch.ops._C_amd.set_tuning("w4_tiled_max_rows", HUGE)
        y_routed = torch.ops._C_amd.skinny_linear_w4a16(x, w4, meta, N, K, G, None)
        torch.ops._C_amd.set_tuning("w4_tiled_min_rows", HUGE)
        y_library = torch.ops._C_amd.skinny_linear_w4a16(x, w4, meta, N, K, G, None)
    finally:
        torch.ops._C_amd.set_tuning("w4_tiled_min_rows", lo)
        torch.ops._C_amd.set_tuning("w4_tiled_max_rows", hi)
    assert torch.equal(y_tiled, y_routed)
    for y in (y_tiled, y_library):
        ok, info = close(y, ref, dtype)
        assert ok, info


@pytest.mark.parametrize("N,K,G", [(16, 192, 64), (24, 128, 128), (16, 128, 16)])
def test_c_entry_returns_3_outside_the_envelope(ops, N, K, G):
    from light_vllm_amd import _native
    lib = _native.load_hip_library()
    lib.lvllm_gemm_w4a16.restype = ctypes.c_int
    M = 8
    x = torch.zeros(M, K, dtype=torch.float16, device=DEV)
    w4 = torch.zeros(4 * 256, dtype=torch.int32, device=DEV)  # two n-tiles x two k-blocks: more than any case needs
    meta = torch.zeros(4 * 16 * 8, dtype=torch.int32, device=DEV)
    y = torch.full((M, N), 7.0, dtype=torch.float16, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.lvllm_gemm_w4a16(p(y), p(x), p(w4), p(meta), None, M, N, K, G, ctypes.c_int64(K), 1, None,
                              ctypes.c_int64(0), None)
    torch.cuda.synchronize()
    assert rc == 3
    assert (y == 7.0).all()
