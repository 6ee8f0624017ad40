"""LDS-tiled bf16 GEMM with fused epilogues (_C_amd.linear_tiled, csrc/dense_tiled_gemm.hip) against torch (hipBLASLt)
on the prefill shapes of bge-m3 and Llama-3-8B, both routes alternating in one process: trains of 8 launches between
device events, weights rotated through HBM, median and spread of 7 trains.  For GELU / SwiGLU the library route is
F.linear followed by the separate activation launch of this build.

  python tools/bench_dense_tiled_gemm.py             all shapes
  python tools/bench_dense_tiled_gemm.py --encoder   also the bge-m3 encoder once with tiled_mlp on and once off"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import light_vllm_amd  # noqa
from light_vllm_amd import _custom_ops as ops

dev = "cuda:0"
TRAIN, REPS = 8, 7
amd = torch.ops._C_amd

SHAPES = [("bge fc1", 4096, 1024, 1, (2048, 16384)), ("bge fc2", 1024, 4096, 0, (2048, 16384)),
          ("8B gate_up", 28672, 4096, 2, (512, 2048, 8192)), ("8B down", 4096, 14336, 0, (512, 2048, 8192)),
          ("8B qkv", 6144, 4096, 0, (512, 2048, 8192))]


def train_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(TRAIN):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / TRAIN


def alternate(fns):
    """median, min, max us per launch of each route, the routes taking turns train by train"""
    for f in fns:
        train_us(f)  # warm-up: code objects, the library's algorithm choice
    ts = [[] for _ in fns]
    for _ in range(REPS):
        for k, f in enumerate(fns):
            ts[k].append(train_us(f))
    return [(sorted(t)[REPS // 2], min(t), max(t)) for t in ts]


def library(x, w, bias, act):
    y = F.linear(x, w, bias)
    if act == 1:
        amd.gelu(y, y)
    elif act == 2:
        out = torch.empty(y.shape[0], y.shape[1] // 2, dtype=y.dtype, device=y.device)
        ops.silu_and_mul(out, y)
        return out
    return y


def gemms():
    for name, N, K, act, Ms in SHAPES:
        nw = max(2, min(4, int(1.0e9 // (N * K * 2))))
        ws = [(torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16) for _ in range(nw)]
        wp = [amd.pack_weight(w) for w in ws]
        bias = None if act == 2 else (torch.randn(N, device=dev) * 0.1).to(torch.bfloat16)
        for M in Ms:
            x = (torch.randn(M, K, device=dev) * 0.5).to(torch.bfloat16)
            (t, tlo, thi), (l, llo, lhi) = alternate([lambda i: amd.linear_tiled(x, wp[i % nw], bias, N, K, act),
                                                      lambda i: library(x, ws[i % nw], bias, act)])
            tf = 2.0 * M * N * K / 1e6
            print(f"{name:10s} act {act} M {M:6d}  tiled {t:8.1f} us [{tlo:.1f} .. {thi:.1f}] {tf / t:6.1f} Tflop/s   "
                  f"library {l:8.1f} us [{llo:.1f} .. {lhi:.1f}] {tf / l:6.1f} Tflop/s   library / tiled {l / t:.3f}",
                  flush=True)
        del ws, wp
        torch.cuda.empty_cache()


def encoder(tokens=16384, seqs=32):
    import dataclasses
    from light_vllm_amd.prefill_only.engine import PrefillOnlyWorker
    from light_vllm_amd.prefill_only.model import EncoderConfig
    ids = torch.randint(2, 250000, (tokens,), generator=torch.Generator().manual_seed(0))
    lo, hi = amd.get_tuning("dense_tiled_min_rows"), amd.get_tuning("dense_tiled_max_rows")
    amd.set_tuning("dense_tiled_min_rows", 65)
    amd.set_tuning("dense_tiled_max_rows", 1 << 30)
    try:
        workers = [PrefillOnlyWorker(dataclasses.replace(EncoderConfig.bge_m3(), tiled_mlp=on), dev, "cls", seed=0)
                   for on in (True, False)]
        mis = [w.build(ids, [tokens // seqs] * seqs) for w in workers]

        def step(k):
            workers[k].execute(mis[k])

        global TRAIN
        TRAIN = 2
        (t, tlo, thi), (l, llo, lhi) = alternate([lambda i: step(0), lambda i: step(1)])
        print(f"bge-m3 encoder, {seqs} x {tokens // seqs} tokens: tiled_mlp on {t / 1e3:.2f} ms [{tlo / 1e3:.2f} .. "
              f"{thi / 1e3:.2f}]   off {l / 1e3:.2f} ms [{llo / 1e3:.2f} .. {lhi / 1e3:.2f}]   off / on {l / t:.3f}")
    finally:
        amd.set_tuning("dense_tiled_min_rows", lo)
        amd.set_tuning("dense_tiled_max_rows", hi)


if __name__ == "__main__":
    gemms()
    if "--encoder" in sys.argv:
        encoder()
