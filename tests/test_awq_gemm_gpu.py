"""W4A16 (AWQ int4) on the GPU (csrc/awq_gemm.hip): dequantisation bit-exact against a torch restatement of the
checkpoint semantics, the weight-streaming GEMM against the fp32 matmul of the dequantised weight (tolerance of the
kernel family, tests/test_skinny_gemm_gpu.py: output rounding + accumulation order; Wd itself is exact)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
ORDER = [0, 2, 4, 6, 1, 3, 5, 7]


def checkpoint(K, N, G, dtype, seed):
    """Random checkpoint tensors (q and z over all of 0..15, positive scales of mixed magnitude) and their Wd."""
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
    return pack(q), pack(z), s, wd


def close(y, ref, dtype):
    err, scale = (y.float() - ref).abs().max().item(), ref.abs().max().item()
    return err <= (2 ** -7 if dtype == torch.bfloat16 else 2 ** -9) * scale + 1e-3, (err, scale)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,N,G", [(128, 16, 128), (256, 48, 64), (384, 64, 32)])
def test_dequantize_and_pack_are_bit_exact(ops, dtype, K, N, G):
    qw, qz, s, wd = checkpoint(K, N, G, dtype, K + N)
    assert torch.equal(ops.awq_dequantize(qw, s, qz, 0, 0, 0), wd)
    # one non-zero product per output: no accumulation error, every nibble of the packed order is pinned
    w4, meta = torch.ops._C_amd.awq_pack(qw, qz, s)
    x = torch.eye(64, K, device=DEV, dtype=dtype)
    assert torch.equal(torch.ops._C_amd.skinny_linear_w4a16(x, w4, meta, N, K, G, None), wd[:64])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("use_bias", [False, True])
@pytest.mark.parametrize("M,N,K,G,wgs", [(1, 16, 128, 128, 0), (5, 48, 256, 64, 0), (17, 64, 384, 128, 0),
                                         (33, 32, 4224, 128, 0), (64, 272, 1024, 32, 0), (64, 272, 1024, 32, 9),
                                         # 16 k-steps per wave: three k-blocks of four (the fourth masked) with two
                                         # m-tiles; four k-blocks with one m-tile and two tiles per meeting
                                         (17, 32, 3072, 32, 0), (32, 80, 3072, 64, 0), (1, 48, 4096, 128, 0)])
def test_w4a16_matches_fp32_matmul(ops, dtype, use_bias, M, N, K, G, wgs):
    qw, qz, s, wd = checkpoint(K, N, G, dtype, M + N + K)
    g = torch.Generator(device=DEV).manual_seed(M)
    x = (torch.randn(M, K, generator=g, device=DEV) * 0.5).to(dtype)
    b = (torch.randn(N, generator=g, device=DEV) * 0.5).to(dtype) if use_bias else None
    w4, meta = torch.ops._C_amd.awq_pack(qw, qz, s)
    default = torch.ops._C_amd.get_tuning("gemm_workgroups")
    try:
        if wgs:
            torch.ops._C_amd.set_tuning("gemm_workgroups", wgs)
        y = torch.ops._C_amd.skinny_linear_w4a16(x, w4, meta, N, K, G, b)
    finally:
        torch.ops._C_amd.set_tuning("gemm_workgroups", default)
    ref = x.float() @ wd.float() + (b.float() if use_bias else 0)
    assert y.shape == (M, N) and y.dtype == dtype
    ok, info = close(y, ref, dtype)
    assert ok, info


def test_strided_rows(ops):
    qw, qz, s, wd = checkpoint(512, 64, 128, torch.bfloat16, 1)
    g = torch.Generator(device=DEV).manual_seed(0)
    big = (torch.randn(8, 3 * 512, generator=g, device=DEV) * 0.5).to(torch.bfloat16)
    x = big[:, 512:1024]  # a column slice: row stride 1536
    w4, meta = torch.ops._C_amd.awq_pack(qw, qz, s)
    ok, info = close(torch.ops._C_amd.skinny_linear_w4a16(x, w4, meta, 64, 512, 128, None), x.float() @ wd.float(),
                     torch.bfloat16)
    assert ok, info


@pytest.mark.parametrize("M,K,G", [(100, 256, 128), (8, 192, 64)])
def test_outside_the_envelope_dequantises_and_multiplies(ops, M, K, G):
    N, dtype = 32, torch.float16
    qw, qz, s, wd = checkpoint(K, N, G, dtype, M + K)
    x = (torch.randn(M, K, generator=torch.Generator(device=DEV).manual_seed(M), device=DEV) * 0.5).to(dtype)
    w4, meta = torch.ops._C_amd.awq_pack(qw, qz, s)
    ref = x.float() @ wd.float()
    for y in (torch.ops._C_amd.skinny_linear_w4a16(x, w4, meta, N, K, G, None), ops.awq_gemm(x, qw, s, qz, 8)):
        ok, info = close(y, ref, dtype)
        assert ok, info
    from light_vllm_amd import _native
    lib = _native.load_hip_library()
    lib.lvllm_skinny_gemm_w4a16.restype = ctypes.c_int
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    y = torch.empty(M, N, device=DEV, dtype=dtype)
    rc = lib.lvllm_skinny_gemm_w4a16(p(y), p(x), p(w4), p(meta), None, M, N, K, G, ctypes.c_int64(K), 1, None,
                                     ctypes.c_int64(0), None)
    assert rc == 3


def test_awq_gemm_equals_the_packed_path_bit_for_bit(ops):
    M, N, K, G, dtype = 7, 48, 256, 64, torch.float16
    qw, qz, s, _ = checkpoint(K, N, G, dtype, 5)
    x = (torch.randn(M, K, generator=torch.Generator(device=DEV).manual_seed(2), device=DEV) * 0.5).to(dtype)
    w4, meta = torch.ops._C_amd.awq_pack(qw, qz, s)
    assert torch.equal(ops.awq_gemm(x, qw, s, qz, 8), torch.ops._C_amd.skinny_linear_w4a16(x, w4, meta, N, K, G, None))
