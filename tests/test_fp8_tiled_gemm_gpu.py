"""LDS-tiled W8A8 fp8 GEMM (csrc/fp8_tiled_gemm.hip) against float64 on the CPU from the same e4m3fn bytes:
ref = acc64 * sx * sw (+ bias).  On the exact grid every fp32 partial sum is exact in any order or split, so acc has one
right value; over the full code range the bound is that of a K-term fp32 sum.  (The MFMA's own 128-term sum is coarser
than an IEEE sum where large products cancel: measured on an MI355X, operands(150, 64, 1536, True) cut to K = 512 has one
accumulator of 9 600 at 1.008 x that bound, profiles/fp8_tiled_gemm.md; the cases below are within it.)"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F8 = torch.float8_e4m3fn


@functools.lru_cache(maxsize=None)
def operands(M, N, K, full_range=False):
    """(xq, wq) fp8 on the CPU, their float64 product and sum_k |x||w|.  Exact grid: multiples of 1/8 in [-1.875,
    1.875] (products multiples of 2^-6, sums below 2^18); full range: every finite e4m3fn code, NaN codes excluded."""
    g = torch.Generator().manual_seed(M + N + K)
    if full_range:
        codes = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=torch.uint8)
        xq = codes[torch.randint(0, 254, (M, K), generator=g)].view(F8)
        wq = codes[torch.randint(0, 254, (N, K), generator=g)].view(F8)
    else:
        xq = (torch.randint(-15, 16, (M, K), generator=g).float() / 8).to(F8)
        wq = (torch.randint(-15, 16, (N, K), generator=g).float() / 8).to(F8)
    x, w = xq.double(), wq.double()
    return xq, wq, x @ w.t(), x.abs() @ w.abs().t()


def reference(acc, sx, sw, bias=None):
    ref = acc * sx.double().reshape(-1, 1) * sw.double().reshape(1, -1)
    return ref if bias is None else ref + bias.double()


def ulp(ref, dtype):
    mant, min_exp = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    return 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** min_exp))) - mant)


def tiled(xq, wq, sx, sw, dtype, bias=None):
    from light_vllm_amd.quantization import pack_fp8_weight
    N, K = wq.shape
    return torch.ops._C_amd.linear_w8a8_fp8_tiled(xq.to(DEV), pack_fp8_weight(wq.to(DEV)), sx.to(DEV), sw.to(DEV), N, K,
                                                  None if bias is None else bias.to(DEV), dtype).cpu()


# The workgroup tile is 128 rows x 128 columns, a K-chunk one MFMA k-step of 128, LDS holds two chunks.
SHAPES = [(1, 16, 64),        # M = 1; one n-tile; K = 64: half a chunk, the other half zero-filled
          (37, 48, 192),      # M no multiple of 16; K / 64 odd: one chunk and a half
          (129, 144, 832),    # one row past a 128-row tile, one n-tile past a 128-column tile; 6 chunks and a half
          (200, 272, 1088),   # 2 x 3 workgroup tiles, 8 chunks and a half
          (130, 32, 8256)]    # 2 tiles on 256 CUs: K split 8 ways, 9 chunks each, the last split one and a half


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("use_bias", [False, True])
@pytest.mark.parametrize("per_row", [False, True])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_tiled_fp8_gemm_on_the_exact_grid(ops, M, N, K, per_row, use_bias, dtype):
    xq, wq, acc, _ = operands(M, N, K)
    g = torch.Generator().manual_seed(N)
    if per_row:  # per-token x per-channel
        sx = (torch.rand(M, generator=g) + 0.5) * 1e-2
        sw = (torch.rand(N, generator=g) + 0.5) * 4.0 ** torch.randint(-3, 3, (N,), generator=g)
    else:        # per-tensor x per-tensor, powers of two
        sx, sw = torch.tensor([2.0 ** -5]), torch.tensor([2.0 ** 2])
    bias = (torch.randn(N, generator=g) * 0.5).to(dtype) if use_bias else None
    y = tiled(xq, wq, sx, sw, dtype, bias)
    ref = reference(acc, sx, sw, bias)
    assert y.shape == (M, N) and y.dtype == dtype
    if not per_row and not use_bias:
        assert torch.equal(y, ref.to(dtype))
    else:
        err = (y.double() - ref).abs() / ulp(ref, dtype)
        assert (err <= 1).all(), err.max().item()


def full_range_bound(acc, mag, sx, sw, bias, K, dtype=torch.bfloat16):
    """(ref, bound): K 2^-24 sum|x||w| sx sw, the bound of a K-term fp32 sum, + 1 ulp of T."""
    ref = reference(acc, sx, sw, bias)
    return ref, K * 2.0 ** -24 * reference(mag, sx, sw) + ulp(ref, dtype)


def test_full_code_range(ops):
    M, N, K = 129, 144, 832
    xq, wq, acc, mag = operands(M, N, K, True)
    g = torch.Generator().manual_seed(1)
    sx = (torch.rand(M, generator=g) + 0.5) * 1e-3 * 4.0 ** torch.randint(-3, 3, (M,), generator=g)
    sw = (torch.rand(N, generator=g) + 0.5) * 1e-2 * 4.0 ** torch.randint(-3, 3, (N,), generator=g)
    bias = (torch.randn(N, generator=g) * 0.5).to(torch.bfloat16)
    ref, bound = full_range_bound(acc, mag, sx, sw, bias, K)
    err = (tiled(xq, wq, sx, sw, torch.bfloat16, bias).double() - ref).abs()
    assert (err <= bound).all(), (err / bound).max().item()


def test_cutlass_scaled_mm_serves_fp8(ops):
    """Inside the envelope the tiled kernel itself (rows of `a` strided), outside it the float64 route."""
    from light_vllm_amd.quantization import pack_fp8_weight
    M, N, K, dtype = 150, 64, 512, torch.bfloat16
    xq, wq, _, _ = operands(M, N, 3 * K, True)
    a, wq = xq.to(DEV)[:, K:2 * K], wq[:, :K].contiguous().to(DEV)
    g = torch.Generator().manual_seed(2)
    sx, sw = (torch.rand(M, 1, generator=g) + 0.5).to(DEV), ((torch.rand(N, 1, generator=g) + 0.5) * 1e-2).to(DEV)
    y = ops.cutlass_scaled_mm(a, wq.t(), sx, sw, dtype)
    assert torch.equal(y, torch.ops._C_amd.linear_w8a8_fp8_tiled(a, pack_fp8_weight(wq), sx, sw, N, K, None, dtype))
    assert torch.equal(y, torch.ops._C_amd.linear_w8a8_fp8_tiled(a.contiguous(), pack_fp8_weight(wq), sx, sw, N, K,
                                                                 None, dtype))
    xq, wq, acc, _ = operands(7, 24, 96)
    sx, sw = torch.rand(7, generator=g) + 0.5, torch.rand(24, generator=g) + 0.5
    y = ops.cutlass_scaled_mm(xq.to(DEV), wq.to(DEV).t(), sx.to(DEV), sw.to(DEV), dtype).cpu()
    ref = reference(acc, sx, sw)
    assert ((y.double() - ref).abs() <= ulp(ref, dtype)).all()


@pytest.mark.parametrize("static", [True, False])
def test_apply_fp8_linear_routes_by_row_count(ops, static, monkeypatch):
    """150 rows that are a column slice (row stride 3 K), the row range forced open: the tiled kernel on
    scaled_fp8_quant's own output, torch._scaled_mm not called.  Forced shut the call reaches torch._scaled_mm as
    before (that route takes contiguous rows only), whether or not the torch build serves fp8 there."""
    from light_vllm_amd.quantization import apply_fp8_linear, pack_fp8_weight
    M, N, K = 150, 64, 512
    _, wq, _, _ = operands(M, N, K, True)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(M, 3 * K, generator=g).to(torch.bfloat16).to(DEV)[:, K:2 * K]
    ws, xs = torch.tensor([0.02], device=DEV), torch.tensor([0.01], device=DEV) if static else None
    bias = torch.randn(N, generator=g).to(torch.bfloat16).to(DEV)
    wq = wq.to(DEV)
    get, put = torch.ops._C_amd.get_tuning, torch.ops._C_amd.set_tuning
    lo, hi = get("fp8_tiled_min_rows"), get("fp8_tiled_max_rows")
    library_calls, scaled_mm = [], torch._scaled_mm
    monkeypatch.setattr(torch, "_scaled_mm", lambda *a, **k: library_calls.append(1) or scaled_mm(*a, **k))
    try:
        put("fp8_tiled_min_rows", 65)
        put("fp8_tiled_max_rows", 1 << 30)
        y = apply_fp8_linear(x, wq.t(), ws, input_scale=xs, bias=bias, w_packed=pack_fp8_weight(wq)).cpu()
        assert not library_calls
        put("fp8_tiled_min_rows", 1 << 30)
        try:
            apply_fp8_linear(x.contiguous(), wq.t(), ws, input_scale=xs, bias=bias, w_packed=pack_fp8_weight(wq))
        except RuntimeError:  # a torch build without fp8 _scaled_mm for this GPU
            pass
        assert library_calls == [1]
    finally:
        put("fp8_tiled_min_rows", lo)
        put("fp8_tiled_max_rows", hi)
    xq, sx = ops.scaled_fp8_quant(x.contiguous(), xs)
    xq = xq.cpu()
    acc, mag = xq.double() @ wq.cpu().double().t(), xq.double().abs() @ wq.cpu().double().abs().t()
    ref, bound = full_range_bound(acc, mag, sx.cpu(), ws.cpu(), bias.cpu(), K)
    assert y.shape == (M, N) and ((y.double() - ref).abs() <= bound).all()


@pytest.mark.parametrize("N,K", [(16, 96), (24, 64)])
def test_c_entry_returns_3_outside_the_envelope(ops, N, K):
    from light_vllm_amd import _native
    lib = _native.load_hip_library()
    lib.lvllm_gemm_w8a8_fp8.restype = ctypes.c_int
    M = 8
    x = torch.zeros(M, K, dtype=torch.uint8, device=DEV)
    w = torch.zeros(N, K, dtype=torch.uint8, device=DEV)
    sx, sw = torch.ones(M, device=DEV), torch.ones(N, device=DEV)
    y = torch.full((M, N), 7.0, dtype=torch.float16, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.lvllm_gemm_w8a8_fp8(p(y), p(x), p(w), p(sx), p(sw), M, N, None, M, N, K, ctypes.c_int64(K), 1, None,
                                 ctypes.c_int64(0), None)
    torch.cuda.synchronize()
    assert rc == 3
    assert (y == 7.0).all()
