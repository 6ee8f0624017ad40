"""Decode-GEMM micro-benchmark: weight-streaming kernel vs torch (hipBLASLt) on the projection
shapes of Llama-3-8B at M = 32; weights rotated so every launch streams from HBM."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import light_vllm_amd  # noqa
from light_vllm_amd import _custom_ops  # noqa

dev = "cuda:0"


def awq_leg(out_path):
    """--awq [out.md]: the W4A16 launch against the bf16 packed launch of the same shape, same process, G = 128.
    Weights rotate through > 1 GB of buffers per format (beyond L2 and the 256 MB last-level cache), 5 warm-up
    launches, then REGIONS regions of PER launches each, the two formats alternating launch by launch inside a region;
    a region's figure is the median of its device-event times, and every region is listed."""
    REGIONS, PER, G = 5, 40, 128
    shapes = [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate_up", 28672, 4096), ("down", 4096, 14336)]
    lines = ["| shape | M | W4A16 us (regions) | bf16 packed us (regions) | W4A16 graph us | bf16 graph us | W4 bytes | "
             "W4 TB/s | bf16 TB/s | speed-up |", "|---|---|---|---|---|---|---|---|---|---|"]
    for name, N, K in shapes:
        qw = torch.randint(-2 ** 31, 2 ** 31, (K, N // 8), device=dev, dtype=torch.int64).to(torch.int32)
        qz = torch.randint(-2 ** 31, 2 ** 31, (K // G, N // 8), device=dev, dtype=torch.int64).to(torch.int32)
        sc = (torch.rand(K // G, N, device=dev) * 0.01 + 1e-3).to(torch.bfloat16)
        w4, meta = torch.ops._C_amd.awq_pack(qw, qz, sc)
        w16 = torch.ops._C_amd.pack_weight((torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16))
        b4, b16 = w4.numel() * 4 + meta.numel() * 4, N * K * 2
        n4, n16 = min(160, int(1.1e9 // b4) + 1), int(1.1e9 // b16) + 1
        w4s, w16s = [(w4.clone(), meta.clone()) for _ in range(n4)], [w16.clone() for _ in range(n16)]
        del qw, qz
        for M in (1, 32, 64):
            x = (torch.randn(M, K, device=dev) * 0.5).to(torch.bfloat16)
            f4 = lambda i: torch.ops._C_amd.skinny_linear_w4a16(x, w4s[i % n4][0], w4s[i % n4][1], N, K, G, None)  # noqa: E731
            f16 = lambda i: torch.ops._C_amd.skinny_linear_packed(x, w16s[i % n16], None, N, K)  # noqa: E731
            for i in range(5):
                f4(i); f16(i)
            torch.cuda.synchronize()
            r4, r16, it = [], [], 0
            for _ in range(REGIONS):
                evs = []
                for _ in range(PER):
                    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                    e[0].record(); f4(it); e[1].record(); f16(it); e[2].record()
                    evs.append(e); it += 1
                torch.cuda.synchronize()
                r4.append(sorted(e[0].elapsed_time(e[1]) * 1e3 for e in evs)[PER // 2])
                r16.append(sorted(e[1].elapsed_time(e[2]) * 1e3 for e in evs)[PER // 2])
            # the same launches without the host in the loop: one captured graph per format that walks every buffer
            # once, replayed REGIONS times; us per launch = replay time / launches (min-max over the replays)
            def replayed(fn, n):
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    for i in range(n):
                        fn(i)
                graph.replay()
                torch.cuda.synchronize()
                ts = []
                for _ in range(REGIONS):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(); graph.replay(); b.record()
                    torch.cuda.synchronize()
                    ts.append(a.elapsed_time(b) * 1e3 / n)
                return ts
            g4, g16 = replayed(f4, n4), replayed(f16, n16)
            xy = M * K * 2 + M * N * 2
            m4, m16 = sorted(r4)[REGIONS // 2], sorted(r16)[REGIONS // 2]
            fmt = lambda r: " ".join(f"{t:.1f}" for t in r)  # noqa: E731
            verdict = "faster beyond the spread" if max(r4) < min(r16) else "NOT faster beyond the spread"
            lines.append(f"| {name} {N}x{K} | {M} | {m4:.1f} ({fmt(r4)}) | {m16:.1f} ({fmt(r16)}) | "
                         f"{min(g4):.1f}-{max(g4):.1f} | {min(g16):.1f}-{max(g16):.1f} | {b4 + xy} | "
                         f"{(b4 + xy) / m4 / 1e6:.2f} | {(b16 + xy) / m16 / 1e6:.2f} | {m16 / m4:.2f}x, {verdict} |")
            print(lines[-1], flush=True)
        del w4s, w16s
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def int8_leg(out_path):
    """--int8 [out.md]: the W8A8 int8 launch (pre-quantised activations, per-token x per-channel scales) against the
    fp8 launch on pre-quantised activations (skinny_linear_w8a8_q: the same bytes per weight; it serves <= 32 rows, the
    M = 64 column stays empty) and the bf16 packed launch, same process.  Weights rotate through > 1 GB of buffers per
    format, 5 warm-up launches, then REGIONS regions of PER launches each, the formats alternating launch by launch
    inside a region; a region's figure is the median of its device-event times, and every region is listed.  Then the
    activation quantisation kernels alone, 32 rows of bf16 at H = 4096 and 14336."""
    import os
    REGIONS, PER = 5, 40
    shapes = [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate_up", 28672, 4096), ("down", 4096, 14336)]
    fmt = lambda r: " ".join(f"{t:.1f}" for t in r)  # noqa: E731
    med = lambda r: sorted(r)[len(r) // 2]  # noqa: E731
    lines = [f"LVLLM_I8_STEPS={os.environ.get('LVLLM_I8_STEPS', '8')} "
             f"LVLLM_I8_INFLIGHT={os.environ.get('LVLLM_I8_INFLIGHT', '8')}", "",
             "| shape | M | int8 us (regions) | fp8 q us (regions) | bf16 packed us (regions) | int8 TB/s | fp8 TB/s | "
             "bf16 TB/s | int8 vs fp8 |", "|---|---|---|---|---|---|---|---|---|"]
    one = torch.ones(1, device=dev)
    for name, N, K in shapes:
        w8 = torch.ops._C_amd.int8_pack(torch.randint(-128, 128, (N, K), device=dev, dtype=torch.int8))
        w16 = torch.ops._C_amd.pack_weight((torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16))
        sw = torch.rand(N, device=dev) * 1e-3 + 1e-4
        n8, n16 = int(1.1e9 // (N * K)) + 1, int(1.1e9 // (N * K * 2)) + 1
        w8s, w16s = [w8.clone() for _ in range(n8)], [w16.clone() for _ in range(n16)]
        wf8s = [w.view(torch.uint8) for w in w8s]  # the fp8 launch streams the same buffers: any byte is an fp8 value
        for M in (1, 32, 64):
            xq = torch.randint(-128, 128, (M, K), device=dev, dtype=torch.int8)
            x8 = torch.randint(0, 120, (M, K), device=dev, dtype=torch.uint8).view(torch.float8_e4m3fn)  # finite values
            x16 = (torch.randn(M, K, device=dev) * 0.5).to(torch.bfloat16)
            sx = torch.rand(M, device=dev) * 1e-2 + 1e-3
            fs = [lambda i: torch.ops._C_amd.skinny_linear_w8a8_int8(xq, w8s[i % n8], sx, sw, N, K, None, torch.bfloat16)]
            if M <= 32:
                fs.append(lambda i: torch.ops._C_amd.skinny_linear_w8a8_q(x8, wf8s[i % n8], one, one, N, K, None,
                                                                          torch.bfloat16))
            fs.append(lambda i: torch.ops._C_amd.skinny_linear_packed(x16, w16s[i % n16], None, N, K))
            for i in range(5):
                for f in fs:
                    f(i)
            torch.cuda.synchronize()
            regions, it = [[] for _ in fs], 0
            for _ in range(REGIONS):
                evs = []
                for _ in range(PER):
                    e = [torch.cuda.Event(enable_timing=True) for _ in range(len(fs) + 1)]
                    e[0].record()
                    for j, f in enumerate(fs):
                        f(it)
                        e[j + 1].record()
                    evs.append(e)
                    it += 1
                torch.cuda.synchronize()
                for j in range(len(fs)):
                    regions[j].append(med([e[j].elapsed_time(e[j + 1]) * 1e3 for e in evs]))
            r8, r16 = regions[0], regions[-1]
            rf = regions[1] if M <= 32 else None
            b8 = N * K + M * K + M * N * 2 + 4 * (M + N)
            b16 = N * K * 2 + M * K * 2 + M * N * 2
            if rf is None:
                verdict = ""
            elif min(r8) > max(rf):
                verdict = f"{med(r8) / med(rf):.2f}x the time, SLOWER beyond the spread"
            elif max(r8) < min(rf):
                verdict = f"{med(r8) / med(rf):.2f}x the time, faster beyond the spread"
            else:
                verdict = f"{med(r8) / med(rf):.2f}x the time, within the spread"
            lines.append(f"| {name} {N}x{K} | {M} | {med(r8):.1f} ({fmt(r8)}) | "
                         + (f"{med(rf):.1f} ({fmt(rf)})" if rf else "") + f" | {med(r16):.1f} ({fmt(r16)}) | "
                         f"{b8 / med(r8) / 1e6:.2f} | " + (f"{b8 / med(rf) / 1e6:.2f}" if rf else "") +
                         f" | {b16 / med(r16) / 1e6:.2f} | {verdict} |")
            print(lines[-1], flush=True)
        del w8s, w16s, wf8s
        torch.cuda.empty_cache()
    lines += ["", "| quantisation, 32 rows of bf16 | H | us per call (regions) |", "|---|---|---|"]
    for H in (4096, 14336):
        x = (torch.randn(32, H, device=dev) * 0.5).to(torch.bfloat16)
        q, sd, st = torch.empty(32, H, device=dev, dtype=torch.int8), torch.empty(32, 1, device=dev), one * 0.05
        for label, f in (("dynamic_scaled_int8_quant", lambda: torch.ops._C.dynamic_scaled_int8_quant(q, x, sd)),
                         ("static_scaled_int8_quant", lambda: torch.ops._C.static_scaled_int8_quant(q, x, st))):
            for _ in range(5):
                f()
            torch.cuda.synchronize()
            rs = []
            for _ in range(REGIONS):
                evs = []
                for _ in range(PER):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(); f(); b.record()
                    evs.append((a, b))
                torch.cuda.synchronize()
                rs.append(med([a.elapsed_time(b) * 1e3 for a, b in evs]))
            lines.append(f"| {label} | {H} | {med(rs):.1f} ({fmt(rs)}) |")
            print(lines[-1], flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def int8_prefill_leg(out_path):
    """--int8-prefill [out.md]: (a) the LDS-tiled W8A8 int8 GEMM (linear_w8a8_int8_tiled) against (b) the 64-row chunks
    of the streaming kernel (skinny_linear_w8a8_int8 with int8_tiled_min_rows above M: what the linear did before the
    tiled kernel) and (c) torch.matmul in bf16, what the 16-bit model pays.  Same process, weights rotate through
    > 0.5 GB per format, 3 warm-up rounds, then REGIONS regions of PER rounds, the legs alternating launch by launch
    inside a round; a region's figure is the median of its device-event times and every region is listed.  The tuning
    key is set once, outside the timed spans.  Op/s from 2 M N K.  INT8_PEAK_TOPS=<dense int8 peak> adds the share of
    that peak."""
    REGIONS = 5
    shapes = [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate_up", 28672, 4096), ("down", 4096, 14336)]
    fmt = lambda r: " ".join(f"{t:.0f}" for t in r)  # noqa: E731
    med = lambda r: sorted(r)[len(r) // 2]  # noqa: E731
    peak = float(os.environ.get("INT8_PEAK_TOPS", "0"))
    default_rows = torch.ops._C_amd.get_tuning("int8_tiled_min_rows")
    lines = ["| shape | M | tiled us (regions) | chunks of 64 us (regions) | bf16 matmul us (regions) | tiled Top/s" +
             (" | of peak" if peak else "") + " | chunks Top/s | bf16 Tflop/s | tiled vs chunks |",
             "|---|---|---|---|---|---|---|---|---|" + ("---|" if peak else "")]
    torch.ops._C_amd.set_tuning("int8_tiled_min_rows", 1 << 30)  # skinny_linear_w8a8_int8 = the chunks from here on
    for name, N, K in shapes:
        w8 = torch.ops._C_amd.int8_pack(torch.randint(-128, 128, (N, K), device=dev, dtype=torch.int8))
        n8, n16 = int(0.55e9 // (N * K)) + 1, int(0.55e9 // (N * K * 2)) + 1
        w8s = [w8.clone() for _ in range(n8)]
        w16s = [(torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16) for _ in range(n16)]
        sw = torch.rand(N, device=dev) * 1e-3 + 1e-4
        for M in (128, 256, 512, 2048, 8192):
            PER = 20 if M <= 512 else 6
            xq = torch.randint(-128, 128, (M, K), device=dev, dtype=torch.int8)
            x16 = (torch.randn(M, K, device=dev) * 0.5).to(torch.bfloat16)
            sx = torch.rand(M, device=dev) * 1e-2 + 1e-3
            fs = [lambda i: torch.ops._C_amd.linear_w8a8_int8_tiled(xq, w8s[i % n8], sx, sw, N, K, None, torch.bfloat16),
                  lambda i: torch.ops._C_amd.skinny_linear_w8a8_int8(xq, w8s[i % n8], sx, sw, N, K, None, torch.bfloat16),
                  lambda i: torch.matmul(x16, w16s[i % n16].t())]
            assert torch.equal(fs[0](0), fs[1](0))  # same bits, or no table
            for i in range(3):
                for f in fs:
                    f(i)
            torch.cuda.synchronize()
            regions, it = [[] for _ in fs], 0
            for _ in range(REGIONS):
                evs = []
                for _ in range(PER):
                    e = [torch.cuda.Event(enable_timing=True) for _ in range(len(fs) + 1)]
                    e[0].record()
                    for j, f in enumerate(fs):
                        f(it)
                        e[j + 1].record()
                    evs.append(e)
                    it += 1
                torch.cuda.synchronize()
                for j in range(len(fs)):
                    regions[j].append(med([e[j].elapsed_time(e[j + 1]) * 1e3 for e in evs]))
            rt, rc, rb = regions
            ops = 2.0 * M * N * K
            verdict = ("faster beyond the spread" if max(rt) < min(rc) else
                       "SLOWER beyond the spread" if min(rt) > max(rc) else "within the spread")
            lines.append(f"| {name} {N}x{K} | {M} | {med(rt):.1f} ({fmt(rt)}) | {med(rc):.1f} ({fmt(rc)}) | "
                         f"{med(rb):.1f} ({fmt(rb)}) | {ops / med(rt) / 1e6:.0f}" +
                         (f" | {ops / med(rt) / 1e6 / peak:.0%}" if peak else "") +
                         f" | {ops / med(rc) / 1e6:.0f} | {ops / med(rb) / 1e6:.0f} | {med(rc) / med(rt):.2f}x, {verdict} |")
            print(lines[-1], flush=True)
        del w8s, w16s
        torch.cuda.empty_cache()
    torch.ops._C_amd.set_tuning("int8_tiled_min_rows", default_rows)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def awq_prefill_leg(out_path):
    """--awq-prefill [out.md]: (a) the LDS-tiled W4A16 GEMM (linear_w4a16_tiled) against (b) dequantise-from-packed +
    library GEMM (skinny_linear_w4a16 with w4_tiled_min_rows huge: what the linear did before the tiled kernel) and
    (c) torch.matmul in bf16, what the 16-bit model pays (a goal, not a gate).  G = 128, bf16.  The method of
    --int8-prefill: same process, weights rotate through > 0.5 GB per format, 3 warm-up rounds, then REGIONS regions of
    PER rounds, the legs alternating launch by launch inside a round; a region's figure is the median of its
    device-event times and every region is listed.  The tuning key is set once, outside the timed spans.  Before
    timing, each row asserts the tiled output within the kernel family's tolerance of the library route's."""
    REGIONS, G = 5, 128
    shapes = [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate_up", 28672, 4096), ("down", 4096, 14336)]
    fmt = lambda r: " ".join(f"{t:.0f}" for t in r)  # noqa: E731
    med = lambda r: sorted(r)[len(r) // 2]  # noqa: E731
    default_rows = torch.ops._C_amd.get_tuning("w4_tiled_min_rows")
    lines = ["| shape | M | tiled us (regions) | dequantise + library us (regions) | bf16 matmul us (regions) | "
             "tiled Tflop/s | dequantise + library Tflop/s | bf16 Tflop/s | tiled vs dequantise + library |",
             "|---|---|---|---|---|---|---|---|---|"]
    torch.ops._C_amd.set_tuning("w4_tiled_min_rows", 1 << 30)  # skinny_linear_w4a16 = the library route from here on
    for name, N, K in shapes:
        qw = torch.randint(-2 ** 31, 2 ** 31, (K, N // 8), device=dev, dtype=torch.int64).to(torch.int32)
        qz = torch.randint(-2 ** 31, 2 ** 31, (K // G, N // 8), device=dev, dtype=torch.int64).to(torch.int32)
        sc = (torch.rand(K // G, N, device=dev) * 0.01 + 1e-3).to(torch.bfloat16)
        w4, meta = torch.ops._C_amd.awq_pack(qw, qz, sc)
        del qw, qz
        n4, n16 = int(0.55e9 // (w4.numel() * 4 + meta.numel() * 4)) + 1, int(0.55e9 // (N * K * 2)) + 1
        w4s = [(w4.clone(), meta.clone()) for _ in range(n4)]
        w16s = [(torch.randn(K, N, device=dev) * 0.02).to(torch.bfloat16) for _ in range(n16)]
        for M in (65, 128, 256, 512, 1024, 2048, 8192):
            PER = 20 if M <= 512 else 6
            x = (torch.randn(M, K, device=dev) * 0.5).to(torch.bfloat16)
            fs = [lambda i: torch.ops._C_amd.linear_w4a16_tiled(x, w4s[i % n4][0], w4s[i % n4][1], N, K, G, None),
                  lambda i: torch.ops._C_amd.skinny_linear_w4a16(x, w4s[i % n4][0], w4s[i % n4][1], N, K, G, None),
                  lambda i: torch.matmul(x, w16s[i % n16])]
            yt, yl = fs[0](0).float(), fs[1](0).float()
            assert (yt - yl).abs().max().item() <= 2 ** -6 * yl.abs().max().item() + 2e-3  # each within 2^-7 + 1e-3 of fp32
            del yt, yl
            for i in range(3):
                for f in fs:
                    f(i)
            torch.cuda.synchronize()
            regions, it = [[] for _ in fs], 0
            for _ in range(REGIONS):
                evs = []
                for _ in range(PER):
                    e = [torch.cuda.Event(enable_timing=True) for _ in range(len(fs) + 1)]
                    e[0].record()
                    for j, f in enumerate(fs):
                        f(it)
                        e[j + 1].record()
                    evs.append(e)
                    it += 1
                torch.cuda.synchronize()
                for j in range(len(fs)):
                    regions[j].append(med([e[j].elapsed_time(e[j + 1]) * 1e3 for e in evs]))
            rt, rl, rb = regions
            flop = 2.0 * M * N * K
            verdict = ("faster beyond the spread" if max(rt) < min(rl) else
                       "SLOWER beyond the spread" if min(rt) > max(rl) else "within the spread")
            lines.append(f"| {name} {N}x{K} | {M} | {med(rt):.1f} ({fmt(rt)}) | {med(rl):.1f} ({fmt(rl)}) | "
                         f"{med(rb):.1f} ({fmt(rb)}) | {flop / med(rt) / 1e6:.0f} | {flop / med(rl) / 1e6:.0f} | "
                         f"{flop / med(rb) / 1e6:.0f} | {med(rl) / med(rt):.2f}x, {verdict} |")
            print(lines[-1], flush=True)
        del w4s, w16s
        torch.cuda.empty_cache()
    torch.ops._C_amd.set_tuning("w4_tiled_min_rows", default_rows)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def fp8_prefill_leg(out_path):
    """--fp8-prefill [out.md]: the W8A8 fp8 linear from bf16 activations, (a) the new route of apply_fp8_linear
    (scaled_fp8_quant without padding + the LDS-tiled kernel, linear_w8a8_fp8_tiled, scales in the epilogue) against
    (b) the route it had before (scaled_fp8_quant padded to 17 rows + torch._scaled_mm, plus the three elementwise
    passes in per-token mode), and (c) the tiled kernel alone on activations quantised beforehand.  Two scale modes:
    static per-tensor x per-tensor (the engine's) and dynamic per-token x per-channel.  The method of --int8-prefill:
    same process, weights rotate through > 0.5 GB per format, 3 warm-up rounds, then REGIONS regions of PER rounds, the
    legs alternating launch by launch inside a round; a region's figure is the median of its device-event times and
    every region is listed.  The tuning keys are set once, outside the timed spans.  Before timing, each row asserts
    the two routes within two bf16 ulps at the output's scale of each other."""
    from light_vllm_amd.quantization import apply_fp8_linear, pack_fp8_weight
    REGIONS = 5
    shapes = [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate_up", 28672, 4096), ("down", 4096, 14336)]
    fmt = lambda r: " ".join(f"{t:.0f}" for t in r)  # noqa: E731
    med = lambda r: sorted(r)[len(r) // 2]  # noqa: E731
    get, put = torch.ops._C_amd.get_tuning, torch.ops._C_amd.set_tuning
    default = get("fp8_tiled_min_rows"), get("fp8_tiled_max_rows")
    lines = ["| scales | shape | M | quantise + tiled us (regions) | quantise + _scaled_mm us (regions) | tiled alone us "
             "(regions) | new route Tflop/s | _scaled_mm route Tflop/s | tiled alone Tflop/s | new vs _scaled_mm route |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    put("fp8_tiled_min_rows", 1)  # with w_packed: always the tiled kernel; without: always the library
    put("fp8_tiled_max_rows", 1 << 30)
    for name, N, K in shapes:
        w8 = torch.randint(0, 120, (N, K), device=dev, dtype=torch.uint8).view(torch.float8_e4m3fn)  # finite values
        n8 = int(0.55e9 // (N * K)) + 1
        wts = [w8.clone().t() for _ in range(n8)]
        wps = [pack_fp8_weight(w.t()) for w in wts]
        for mode in ("per-tensor", "per-token x per-channel"):
            per_token = mode != "per-tensor"
            ws = torch.rand(N, 1, device=dev) * 1e-3 + 1e-4 if per_token else torch.full((1,), 5e-4, device=dev)
            xs = None if per_token else torch.full((1,), 0.01, device=dev)
            for M in (65, 128, 256, 512, 1024, 2048, 8192):
                PER = 20 if M <= 512 else 6
                x = (torch.randn(M, K, device=dev) * 0.5).to(torch.bfloat16)
                xq, sx = _custom_ops.scaled_fp8_quant(x, xs, use_per_token_if_dynamic=per_token)
                fs = [lambda i: apply_fp8_linear(x, wts[i % n8], ws, input_scale=xs, use_per_token_if_dynamic=per_token,
                                                 w_packed=wps[i % n8]),
                      lambda i: apply_fp8_linear(x, wts[i % n8], ws, input_scale=xs, use_per_token_if_dynamic=per_token),
                      lambda i: torch.ops._C_amd.linear_w8a8_fp8_tiled(xq, wps[i % n8], sx, ws, N, K, None, torch.bfloat16)]
                yn, yl = fs[0](0).float(), fs[1](0).float()
                assert torch.equal(fs[0](0), fs[2](0))
                assert (yn - yl).abs().max().item() <= 2 ** -7 * yl.abs().max().item(), (name, mode, M)
                del yn, yl
                for i in range(3):
                    for f in fs:
                        f(i)
                torch.cuda.synchronize()
                regions, it = [[] for _ in fs], 0
                for _ in range(REGIONS):
                    evs = []
                    for _ in range(PER):
                        e = [torch.cuda.Event(enable_timing=True) for _ in range(len(fs) + 1)]
                        e[0].record()
                        for j, f in enumerate(fs):
                            f(it)
                            e[j + 1].record()
                        evs.append(e)
                        it += 1
                    torch.cuda.synchronize()
                    for j in range(len(fs)):
                        regions[j].append(med([e[j].elapsed_time(e[j + 1]) * 1e3 for e in evs]))
                rn, rl, rk = regions
                flop = 2.0 * M * N * K
                verdict = ("faster beyond the spread" if max(rn) < min(rl) else
                           "SLOWER beyond the spread" if min(rn) > max(rl) else "within the spread")
                lines.append(f"| {mode} | {name} {N}x{K} | {M} | {med(rn):.1f} ({fmt(rn)}) | {med(rl):.1f} ({fmt(rl)}) | "
                             f"{med(rk):.1f} ({fmt(rk)}) | {flop / med(rn) / 1e6:.0f} | {flop / med(rl) / 1e6:.0f} | "
                             f"{flop / med(rk) / 1e6:.0f} | {med(rl) / med(rn):.2f}x, {verdict} |")
                print(lines[-1], flush=True)
        del wts, wps
        torch.cuda.empty_cache()
    put("fp8_tiled_min_rows", default[0])
    put("fp8_tiled_max_rows", default[1])
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if len(sys.argv) > 1 and sys.argv[1] == "--fp8-prefill":
    fp8_prefill_leg(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] == "--awq-prefill":
    awq_prefill_leg(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] == "--int8-prefill":
    int8_prefill_leg(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)

def mxfp4_leg(out_path):
    """--mxfp4 [out.md]: the W4A8 MXFP4 launch (fp8 activations quantised beforehand, per-token scales) against the
    fp8 W8A8 decode launch (skinny_linear_w8a8_q on pre-quantised activations up to 32 rows; at 64 rows
    skinny_linear_w8a8, which quantises 16-bit activations in its prologue) and the AWQ W4A16 decode launch (G = 128),
    same process.  The method is the other legs': weights rotate through > 1 GB of buffers per format, 5 warm-up
    launches, REGIONS regions of PER launches, the formats alternating launch by launch; a region's figure is the
    median of its device-event times, every region is listed."""
    REGIONS, PER, G = 5, 40, 128
    shapes = [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate_up", 28672, 4096), ("down", 4096, 14336)]
    fmt = lambda r: " ".join(f"{t:.1f}" for t in r)  # noqa: E731
    med = lambda r: sorted(r)[len(r) // 2]  # noqa: E731
    lines = ["| shape | M | mxfp4 us (regions) | fp8 us (regions) | AWQ us (regions) | mxfp4 TB/s | fp8 TB/s | "
             "AWQ TB/s | mxfp4 vs fp8 | mxfp4 vs AWQ |", "|---|---|---|---|---|---|---|---|---|---|"]
    one = torch.ones(1, device=dev)

    def verdict(a, b):
        word = "SLOWER beyond" if min(a) > max(b) else "faster beyond" if max(a) < min(b) else "within"
        return f"{med(a) / med(b):.2f}x the time, {word} the spread"

    for name, N, K in shapes:
        wp, ep = torch.ops._C_amd.mxfp4_pack(torch.randint(0, 256, (N, K // 2), device=dev, dtype=torch.uint8),
                                             torch.randint(117, 130, (N, K // 32), device=dev, dtype=torch.uint8))
        w8 = torch.ops._C_amd.int8_pack(torch.randint(-120, 120, (N, K), device=dev, dtype=torch.int8)).view(torch.uint8)
        qw = torch.randint(-2 ** 31, 2 ** 31, (K, N // 8), device=dev, dtype=torch.int64).to(torch.int32)
        qz = torch.randint(-2 ** 31, 2 ** 31, (K // G, N // 8), device=dev, dtype=torch.int64).to(torch.int32)
        w4, meta = torch.ops._C_amd.awq_pack(qw, qz, (torch.rand(K // G, N, device=dev) * 0.01 + 1e-3).to(torch.bfloat16))
        del qw, qz
        bmx, b8, b4 = wp.numel() + ep.numel(), N * K, w4.numel() * 4 + meta.numel() * 4
        nmx, n8, n4 = (min(160, int(1.1e9 // b) + 1) for b in (bmx, b8, b4))
        mxs, w8s = [(wp.clone(), ep.clone()) for _ in range(nmx)], [w8.clone() for _ in range(n8)]
        w4s = [(w4.clone(), meta.clone()) for _ in range(n4)]
        for M in (1, 8, 32, 64):
            x8 = torch.randint(0, 120, (M, K), device=dev, dtype=torch.uint8).view(torch.float8_e4m3fn)  # finite values
            x16 = (torch.randn(M, K, device=dev) * 0.5).to(torch.bfloat16)
            sx = torch.rand(M, device=dev) * 1e-2 + 1e-3
            fs = [lambda i: torch.ops._C_amd.skinny_linear_w4a8_mxfp4(x8, mxs[i % nmx][0], mxs[i % nmx][1], sx, N, K, None,
                                                                      torch.bfloat16),
                  (lambda i: torch.ops._C_amd.skinny_linear_w8a8_q(x8, w8s[i % n8], one, one, N, K, None, torch.bfloat16))
                  if M <= 32 else (lambda i: torch.ops._C_amd.skinny_linear_w8a8(x16, w8s[i % n8], one, one, N, K, None)),
                  lambda i: torch.ops._C_amd.skinny_linear_w4a16(x16, w4s[i % n4][0], w4s[i % n4][1], N, K, G, None)]
            for i in range(5):
                for f in fs:
                    f(i)
            torch.cuda.synchronize()
            regions, it = [[] for _ in fs], 0
            for _ in range(REGIONS):
                evs = []
                for _ in range(PER):
                    e = [torch.cuda.Event(enable_timing=True) for _ in range(len(fs) + 1)]
                    e[0].record()
                    for j, f in enumerate(fs):
                        f(it)
                        e[j + 1].record()
                    evs.append(e)
                    it += 1
                torch.cuda.synchronize()
                for j in range(len(fs)):
                    regions[j].append(med([e[j].elapsed_time(e[j + 1]) * 1e3 for e in evs]))
            rmx, r8, r4 = regions
            tot = [bmx + M * K + M * N * 2 + 4 * M, b8 + M * K * (1 if M <= 32 else 2) + M * N * 2,
                   b4 + M * K * 2 + M * N * 2]
            lines.append(f"| {name} {N}x{K} | {M} | {med(rmx):.1f} ({fmt(rmx)}) | {med(r8):.1f} ({fmt(r8)}) | "
                         f"{med(r4):.1f} ({fmt(r4)}) | {tot[0] / med(rmx) / 1e6:.2f} | {tot[1] / med(r8) / 1e6:.2f} | "
                         f"{tot[2] / med(r4) / 1e6:.2f} | {verdict(rmx, r8)} | {verdict(rmx, r4)} |")
            print(lines[-1], flush=True)
        del mxs, w8s, w4s
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def mxfp4_prefill_leg(out_path):
    """--mxfp4-prefill [out.md]: (a) the LDS-tiled W4A8 MXFP4 GEMM (linear_w4a8_mxfp4_tiled) against (b) the 64-row
    chunks of the streaming kernel (skinny_linear_w4a8_mxfp4 with mxfp4_tiled_min_rows huge: what the linear did before
    the tiled kernel) and, for context only, (c) the LDS-tiled W8A8 fp8 GEMM on the same shapes.  bf16 output,
    activations quantised beforehand, per-token scales.  The method of --mxfp4: same process, weights rotate through
    > 1 GB of buffers per format, 5 warm-up launches, then REGIONS regions of PER launches, the legs alternating launch
    by launch; a region's figure is the median of its device-event times and every region is listed.  The tuning key
    is set once, outside the timed spans.  Before timing, each row asserts (a) within two bf16 ulps at the output's
    scale of (b).  The last lines name the smallest M from which (a) is faster beyond the spread on all four shapes
    and stays so."""
    REGIONS, PER = 5, 40
    MS = (65, 128, 256, 512, 1024, 2048, 8192)
    shapes = [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate_up", 28672, 4096), ("down", 4096, 14336)]
    fmt = lambda r: " ".join(f"{t:.0f}" for t in r)  # noqa: E731
    med = lambda r: sorted(r)[len(r) // 2]  # noqa: E731
    get, put = torch.ops._C_amd.get_tuning, torch.ops._C_amd.set_tuning
    default_rows = get("mxfp4_tiled_min_rows")
    lines = ["| shape | M | tiled us (regions) | chunks of 64 us (regions) | fp8 tiled us (regions) | tiled Tflop/s | "
             "chunks Tflop/s | fp8 tiled Tflop/s | tiled vs chunks |", "|---|---|---|---|---|---|---|---|---|"]
    put("mxfp4_tiled_min_rows", 1 << 30)  # skinny_linear_w4a8_mxfp4 = the chunks from here on
    wins = {M: 0 for M in MS}
    one = torch.ones(1, device=dev)
    for name, N, K in shapes:
        wp, ep = torch.ops._C_amd.mxfp4_pack(torch.randint(0, 256, (N, K // 2), device=dev, dtype=torch.uint8),
                                             torch.randint(117, 130, (N, K // 32), device=dev, dtype=torch.uint8))
        w8 = torch.randint(0, 120, (N * K,), device=dev, dtype=torch.uint8)  # packing permutes bytes: any finite ones do
        nmx, n8 = min(160, int(1.1e9 // (wp.numel() + ep.numel())) + 1), int(1.1e9 // (N * K)) + 1
        mxs, w8s = [(wp.clone(), ep.clone()) for _ in range(nmx)], [w8.clone() for _ in range(n8)]
        for M in MS:
            x8 = torch.randint(0, 120, (M, K), device=dev, dtype=torch.uint8).view(torch.float8_e4m3fn)  # finite values
            sx = torch.rand(M, device=dev) * 1e-2 + 1e-3
            fs = [lambda i: torch.ops._C_amd.linear_w4a8_mxfp4_tiled(x8, mxs[i % nmx][0], mxs[i % nmx][1], sx, N, K, None,
                                                                     torch.bfloat16),
                  lambda i: torch.ops._C_amd.skinny_linear_w4a8_mxfp4(x8, mxs[i % nmx][0], mxs[i % nmx][1], sx, N, K, None,
                                                                      torch.bfloat16),
                  lambda i: torch.ops._C_amd.linear_w8a8_fp8_tiled(x8, w8s[i % n8], sx, one, N, K, None, torch.bfloat16)]
            ya, yb = fs[0](0).float(), fs[1](0).float()
            assert (ya - yb).abs().max().item() <= 2 ** -7 * yb.abs().max().item(), (name, M)
            del ya, yb
            for i in range(5):
                for f in fs:
                    f(i)
            torch.cuda.synchronize()
            regions, it = [[] for _ in fs], 0
            for _ in range(REGIONS):
                evs = []
                for _ in range(PER):
                    e = [torch.cuda.Event(enable_timing=True) for _ in range(len(fs) + 1)]
                    e[0].record()
                    for j, f in enumerate(fs):
                        f(it)
                        e[j + 1].record()
                    evs.append(e)
                    it += 1
                torch.cuda.synchronize()
                for j in range(len(fs)):
                    regions[j].append(med([e[j].elapsed_time(e[j + 1]) * 1e3 for e in evs]))
            rt, rc, r8 = regions
            flop = 2.0 * M * N * K
            wins[M] += max(rt) < min(rc)
            verdict = ("faster beyond the spread" if max(rt) < min(rc) else
                       "SLOWER beyond the spread" if min(rt) > max(rc) else "within the spread")
            lines.append(f"| {name} {N}x{K} | {M} | {med(rt):.1f} ({fmt(rt)}) | {med(rc):.1f} ({fmt(rc)}) | "
                         f"{med(r8):.1f} ({fmt(r8)}) | {flop / med(rt) / 1e6:.0f} | {flop / med(rc) / 1e6:.0f} | "
                         f"{flop / med(r8) / 1e6:.0f} | {med(rc) / med(rt):.2f}x, {verdict} |")
            print(lines[-1], flush=True)
        del mxs, w8s
        torch.cuda.empty_cache()
    put("mxfp4_tiled_min_rows", default_rows)
    ahead = [M for i, M in enumerate(MS) if all(wins[m] == len(shapes) for m in MS[i:])]
    lines += ["", f"tiled faster beyond the spread on all {len(shapes)} shapes from M = {ahead[0]} on" if ahead else
              "no M from which the tiled kernel is faster beyond the spread on all shapes and stays so",
              f"mxfp4_tiled_min_rows of this build: {default_rows}"]
    print("\n".join(lines[-2:]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def fp8_block_leg(out_path):
    """--fp8-block [out.md]: the block-scaled W8A8 fp8 launch (skinny_linear_w8a8_fp8_block on activations quantised
    beforehand) against the per-tensor W8A8 launch (skinny_linear_w8a8 on 16-bit activations: the same weight bytes),
    and the per-token-group quantiser on its own.  The method of --mxfp4: same process, weights rotate through > 1 GB
    of buffers per format, 5 warm-up launches, REGIONS regions of PER launches, the legs alternating launch by launch;
    a region's figure is the median of its device-event times, every region is listed."""
    REGIONS, PER = 5, 40
    shapes = [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate_up", 28672, 4096), ("down", 4096, 14336)]
    fmt = lambda r: " ".join(f"{t:.1f}" for t in r)  # noqa: E731
    med = lambda r: sorted(r)[len(r) // 2]  # noqa: E731
    lines = ["| shape | M | block us (regions) | per-tensor us (regions) | quant us (regions) | block TB/s | "
             "per-tensor TB/s | block vs per-tensor |", "|---|---|---|---|---|---|---|---|"]
    one = torch.ones(1, device=dev)
    for name, N, K in shapes:
        w8 = torch.randint(0, 120, (N * K,), device=dev, dtype=torch.uint8)  # both packs permute bytes: any finite ones
        ws = torch.rand((N + 127) // 128, K // 128, device=dev) * 1e-2 + 1e-3
        nw = int(1.1e9 // (N * K)) + 1
        wbs, wts = [w8.clone() for _ in range(nw)], [w8.clone() for _ in range(nw)]
        for M in (1, 8, 32, 64):
            x16 = (torch.randn(M, K, device=dev) * 0.5).to(torch.bfloat16)
            xq, xs = torch.ops._C_amd.per_token_group_fp8_quant(x16)
            fs = [lambda i: torch.ops._C_amd.skinny_linear_w8a8_fp8_block(xq, wbs[i % nw], xs, ws, N, K, None, torch.bfloat16),
                  lambda i: torch.ops._C_amd.skinny_linear_w8a8(x16, wts[i % nw], one, one, N, K, None),
                  lambda i: torch.ops._C_amd.per_token_group_fp8_quant(x16)]
            for i in range(5):
                for f in fs:
                    f(i)
            torch.cuda.synchronize()
            regions, it = [[] for _ in fs], 0
            for _ in range(REGIONS):
                evs = []
                for _ in range(PER):
                    e = [torch.cuda.Event(enable_timing=True) for _ in range(len(fs) + 1)]
                    e[0].record()
                    for j, f in enumerate(fs):
                        f(it)
                        e[j + 1].record()
                    evs.append(e)
                    it += 1
                torch.cuda.synchronize()
                for j in range(len(fs)):
                    regions[j].append(med([e[j].elapsed_time(e[j + 1]) * 1e3 for e in evs]))
            rb, rt, rq = regions
            tot = [N * K + ws.numel() * 4 + M * K + xs.numel() * 4 + M * N * 2, N * K + M * K * 2 + M * N * 2]
            word = "SLOWER beyond" if min(rb) > max(rt) else "faster beyond" if max(rb) < min(rt) else "within"
            lines.append(f"| {name} {N}x{K} | {M} | {med(rb):.1f} ({fmt(rb)}) | {med(rt):.1f} ({fmt(rt)}) | "
                         f"{med(rq):.1f} ({fmt(rq)}) | {tot[0] / med(rb) / 1e6:.2f} | {tot[1] / med(rt) / 1e6:.2f} | "
                         f"{med(rb) / med(rt):.2f}x the time, {word} the spread |")
            print(lines[-1], flush=True)
        del wbs, wts
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if len(sys.argv) > 1 and sys.argv[1] == "--fp8-block":
    fp8_block_leg(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] == "--mxfp4-prefill":
    mxfp4_prefill_leg(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] == "--mxfp4":
    mxfp4_leg(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] == "--int8":
    int8_leg(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] == "--awq":
    awq_leg(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)

M = int(sys.argv[1]) if len(sys.argv) > 1 else 32
for name, N, K in [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate_up", 28672, 4096), ("down", 4096, 14336), ("lm_head", 128256, 4096)]:
    nw = max(2, min(12, int(1.2e9 // (N * K * 2))))
    ws = [(torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16) for _ in range(nw)]
    x = (torch.randn(M, K, device=dev) * 0.5).to(torch.bfloat16)
    res = {}
    for label, fn in (("skinny", lambda w: torch.ops._C_amd.skinny_linear(x, w, None)),
                      ("packed", lambda w: torch.ops._C_amd.skinny_linear_packed(x, w, None, N, K)),
                      ("torch", lambda w: F.linear(x, w))):
        for i in range(5):
            fn(ws[i % nw])
        torch.cuda.synchronize()
        evs = []
        for i in range(60):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(ws[i % nw]); b.record(); evs.append((a, b))
        torch.cuda.synchronize()
        ts = sorted(a.elapsed_time(b) * 1e3 for a, b in evs)
        res[label] = ts[len(ts) // 2]
    by = N * K * 2
    print(f"{name:8s} N={N:6d} K={K:5d}  skinny {res['skinny']:7.1f} us ({by / res['skinny'] / 1e6:5.2f} TB/s)   packed {res['packed']:7.1f} us ({by / res['packed'] / 1e6:5.2f} TB/s)   torch {res['torch']:7.1f} us ({by / res['torch'] / 1e6:5.2f} TB/s)")
