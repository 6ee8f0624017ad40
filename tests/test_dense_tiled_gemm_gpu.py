"""LDS-tiled bf16 / f16 GEMM (csrc/dense_tiled_gemm.hip) against float64 on the CPU from the same 16-bit operands.  On
the exact grid every fp32 partial sum is exact in any order or split, so the accumulator has one right value; on random
operands the bound is that of a K-term fp32 sum plus the output rounding; the fused epilogues must leave the bits of
the unfused sequence."""
import dataclasses
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]


@functools.lru_cache(maxsize=None)
def operands(M, N, K, dtype, grid=True):
    """(x, w, bias) of `dtype` on the CPU, their float64 product and sum_k |x||w|.  Exact grid: multiples of 1/8 in
    [-1.875, 1.875] (products multiples of 2^-6, sums below 2^15 at K <= 8256); otherwise randn rounded to dtype."""
    g = torch.Generator().manual_seed(M + N + K)
    if grid:
        x = (torch.randint(-15, 16, (M, K), generator=g).float() / 8).to(dtype)
        w = (torch.randint(-15, 16, (N, K), generator=g).float() / 8).to(dtype)
    else:
        x = torch.randn(M, K, generator=g).to(dtype)
        w = (torch.randn(N, K, generator=g) * 0.05).to(dtype)
    bias = (torch.randn(N, generator=g) * 0.5).to(dtype)
    return x, w, bias, x.double() @ w.double().t(), x.double().abs() @ w.double().abs().t()


def ulp(ref, dtype):
    mant, min_exp = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    return 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** min_exp))) - mant)


def tiled(x, w, bias=None, act=0):
    N, K = w.shape
    return torch.ops._C_amd.linear_tiled(x.to(DEV), torch.ops._C_amd.pack_weight(w.to(DEV)),
                                         None if bias is None else bias.to(DEV), N, K, act)


# The workgroup tile is 128 rows x 128 columns, a K-chunk 64 elements (two MFMA k-steps), LDS holds two chunks.
SHAPES = [(1, 16, 32),        # one row, one n-tile, half a chunk (the other half zero-filled)
          (37, 48, 96),       # M no multiple of 16; K / 32 odd: one chunk and a half
          (129, 144, 832),    # one row past a 128-row tile, one n-tile past a 128-column tile
          (200, 272, 1056),   # 2 x 3 workgroup tiles, a trailing half chunk
          (130, 32, 8256)]    # 2 tiles on 256 CUs: K is split, and the last split ends on a half chunk


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("use_bias", [False, True])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_exact_grid(ops, M, N, K, use_bias, dtype):
    x, w, bias, acc, _ = operands(M, N, K, dtype)
    y = tiled(x, w, bias if use_bias else None).cpu()
    assert y.shape == (M, N) and y.dtype == dtype
    if not use_bias:
        assert torch.equal(y, acc.to(dtype))
    else:
        ref = acc + bias.double()
        err = (y.double() - ref).abs() / ulp(ref, dtype)
        assert (err <= 1).all(), err.max().item()


def test_strided_rows_equal_contiguous_rows(ops):
    M, N, K = 129, 144, 832
    x, w, bias, _, _ = operands(M, N, 3 * K, torch.bfloat16)
    a, w = x.to(DEV)[:, K:2 * K], w[:, :K].contiguous()  # ldx = 3 K
    assert torch.equal(tiled(a, w, bias), tiled(a.contiguous(), w, bias))


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_operands_within_the_fp32_sum_bound(ops, dtype):
    M, N, K = 129, 144, 832
    x, w, bias, acc, mag = operands(M, N, K, dtype, False)
    ref = acc + bias.double()
    bound = K * 2.0 ** -24 * mag + ulp(ref, dtype)  # a K-term fp32 sum, then one rounding to T
    err = (tiled(x, w, bias).cpu().double() - ref).abs()
    print(f"{dtype}: max err / bound = {(err / bound).max().item():.4f}")
    assert (err <= bound).all(), (err / bound).max().item()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act,M,N,K", [(1, 129, 144, 832),
                                       (2, 129, 288, 832),  # gate and up n-tiles cross a partial workgroup tile
                                       (2, 1, 32, 32)])
def test_fused_epilogue_is_the_unfused_sequence(ops, act, M, N, K, dtype):
    x, w, bias, _, _ = operands(M, N, K, dtype, False)
    y = tiled(x, w, bias, 0)
    if act == 1:
        want = torch.empty_like(y)
        torch.ops._C_amd.gelu(want, y)
    else:
        want = torch.empty(M, N // 2, dtype=dtype, device=DEV)
        ops.silu_and_mul(want, y)
    got = tiled(x, w, bias, act)
    assert got.shape == want.shape and torch.equal(got, want)


@pytest.fixture
def open_row_range():
    get, put = torch.ops._C_amd.get_tuning, torch.ops._C_amd.set_tuning
    lo, hi = get("dense_tiled_min_rows"), get("dense_tiled_max_rows")
    try:
        put("dense_tiled_min_rows", 65)
        put("dense_tiled_max_rows", 1 << 30)
        yield
    finally:
        put("dense_tiled_min_rows", lo)
        put("dense_tiled_max_rows", hi)


def test_decoder_linear_takes_the_tiled_kernel(ops, open_row_range, monkeypatch):
    from light_vllm_amd.engine.model import Weight, linear
    x, w, bias, _, _ = operands(130, 144, 832, torch.bfloat16, False)
    weight = Weight(w.to(DEV))
    want = torch.ops._C_amd.linear_tiled(x.to(DEV), weight.packed, bias.to(DEV), 144, 832, 0)
    acts, op = [], torch.ops._C_amd.linear_tiled
    monkeypatch.setattr(torch.ops._C_amd, "linear_tiled", lambda *a: acts.append(a[-1]) or op(*a))
    y = linear(x.to(DEV), weight, bias.to(DEV))
    assert acts == [0] and torch.equal(y, want)


def encoder_float64(model, ids):
    """float64 torch forward of EncoderModel's weights on one sequence, dense bidirectional attention."""
    import torch.nn.functional as F
    cfg = model.cfg
    hid, H, D, eps = cfg.hidden_size, cfg.num_attention_heads, cfg.head_dim, cfg.layer_norm_eps
    T = ids.numel()
    f = lambda t: t.double()  # noqa: E731
    ln = lambda t, p: F.layer_norm(t, (hid,), f(p[0]), f(p[1]), eps)  # noqa: E731
    pos = torch.arange(T, device=ids.device) + cfg.pad_token_id + 1
    x = ln(f(model.word_emb)[ids] + f(model.pos_emb)[pos] + f(model.type_emb)[0], model.emb_ln)
    for lw in model.layers:
        qkv = x @ f(lw.qkv_w).T + f(lw.qkv_b)
        q, k, v = (t.view(T, H, D).transpose(0, 1) for t in qkv.split([hid, hid, hid], dim=-1))
        a = (torch.softmax(q @ k.transpose(1, 2) / D ** 0.5, dim=-1) @ v).transpose(0, 1).reshape(T, hid)
        x = ln(x + a @ f(lw.out_w).T + f(lw.out_b), lw.attn_ln)
        x = ln(x + F.gelu(x @ f(lw.fc1_w).T + f(lw.fc1_b)) @ f(lw.fc2_w).T + f(lw.fc2_b), lw.out_ln)
    return x


def test_encoder_tiled_mlp_is_as_close_to_float64_as_the_library_route(ops, open_row_range, monkeypatch):
    """200 tokens of the tiny encoder: both routes round the same mathematics once per op, the factor 2 is the margin
    for the other summation order.  With the flag on, fc1 + GELU and fc2 of both layers are tiled launches."""
    from light_vllm_amd.prefill_only.engine import PrefillOnlyWorker
    from light_vllm_amd.prefill_only.model import EncoderConfig
    ids = torch.randint(2, 512, (200,), generator=torch.Generator().manual_seed(1))
    acts, op = [], torch.ops._C_amd.linear_tiled
    monkeypatch.setattr(torch.ops._C_amd, "linear_tiled", lambda *a: acts.append(a[-1]) or op(*a))
    dist = {}
    for tiled_mlp in (True, False):
        worker = PrefillOnlyWorker(dataclasses.replace(EncoderConfig.tiny(), tiled_mlp=tiled_mlp), DEV,
                                   "last_hidden_states", seed=0)
        got = worker.execute(worker.build(ids, [200]))
        torch.cuda.synchronize()
        assert acts == [1, 0, 1, 0]  # the flag on: four tiled launches; the flag off adds none
        err = (got.double() - encoder_float64(worker.model, ids.to(DEV)).cpu()).abs()
        dist[tiled_mlp] = (err.max().item(), err.mean().item())
    print(f"|y - float64| (max, mean): tiled_mlp {dist[True]}, library {dist[False]}")
    assert dist[True][0] <= 2 * dist[False][0] and dist[True][1] <= 2 * dist[False][1]
