"""Micro-benchmark for the KV-cache prefill attention kernel at Llama-3-8B
head shapes (Hq 32, Hkv 8, D 128).

Usage: python tools/prefill_bench.py [--iters N] [--warmup N] [--batch B]
                                     [--mem-batch B]

Times the attention op only (device events, median over --iters) for three
cases — a ragged prompt (pos=0, s=1000), an aligned prompt (pos=0, s=1024)
and a chunk against a long prefix (pos=3000, s=256) — with bf16 and fp8
caches. Next to each it times the fp32 fallback the models used before the
kernel existed (dequantise the prefix + reference.attention_cached) on the
same GPU tensors, and for s=1024 the aligned flash_attention kernel. Ends
with the peak memory of one s=1000 call through either path.
"""

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

HQ, HKV, D = 32, 8, 128
CASES = [(0, 1000), (0, 1024), (3000, 256)]  # (pos, s)


def event_time_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def causal_flops(b, pos, s):
    # QK^T + PV over the visible (q, kv) pairs: sum_i (pos + i + 1)
    pairs = s * pos + s * (s + 1) // 2
    return 2 * 2 * b * HQ * pairs * D


def peak_mem_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--batch", type=int, default=1)
    p.add_argument("--mem-batch", type=int, default=8,
                   help="batch of the peak-memory comparison (0 = skip)")
    args = p.parse_args()

    from hypha_amd import ops
    from hypha_amd.models.kv_cache import KVCache

    assert torch.cuda.is_available(), "prefill_bench needs a GPU"
    ops.native_available_or_raise()
    dev = "cuda:0"
    torch.manual_seed(0)

    def make(b, pos, s, quant):
        t = pos + s
        q = torch.randn(b, s, HQ, D, device=dev).bfloat16()
        k = torch.randn(b, t, HKV, D, device=dev).bfloat16()
        v = torch.randn(b, t, HKV, D, device=dev).bfloat16()
        cache = KVCache(b, t, HKV, D, dev, quant=quant)
        cache.append(k, v)
        return q, k, v, cache

    def kernel(q, cache, pos):
        return ops.attn_prefill(q, cache.k, cache.v, pos, cache.k_scale, cache.v_scale)

    def fallback(q, cache, pos):
        kc, vc = cache.dequant(pos + q.shape[1])
        return ops.reference.attention_cached(q, kc, vc, pos)

    B = args.batch
    for pos, s in CASES:
        for quant in (None, "fp8"):
            q, k, v, cache = make(B, pos, s, quant)
            err = (kernel(q, cache, pos).float()
                   - fallback(q, cache, pos).float()).abs().max().item()
            t_k = event_time_ms(lambda: kernel(q, cache, pos), args.warmup, args.iters)
            t_r = event_time_ms(lambda: fallback(q, cache, pos), args.warmup, args.iters)
            row = {"case": f"pos={pos} s={s}", "batch": B, "cache": quant or "bf16",
                   "prefill_ms": round(t_k, 4), "reference_ms": round(t_r, 4),
                   "speedup_vs_reference": round(t_r / t_k, 2),
                   "prefill_tflops": round(causal_flops(B, pos, s) / t_k / 1e9, 1),
                   "max_abs_diff_vs_reference": round(err, 5)}
            if pos == 0 and s % 128 == 0 and quant is None:
                t_f = event_time_ms(
                    lambda: ops.flash_attention(q, k, v, causal=True, layout="bshd"),
                    args.warmup, args.iters)
                row["flash_ms"] = round(t_f, 4)
                row["prefill_over_flash"] = round(t_k / t_f, 3)
            print(json.dumps(row), flush=True)
            del q, k, v, cache

    if args.mem_batch > 0:
        for b in sorted({1, args.mem_batch}):
            q, k, v, cache = make(b, 0, 1000, None)
            row = {"case": "peak memory, pos=0 s=1000, bf16 cache", "batch": b,
                   "prefill_peak_mb": round(peak_mem_mb(lambda: kernel(q, cache, 0)), 1),
                   "reference_peak_mb": round(
                       peak_mem_mb(lambda: fallback(q, cache, 0)), 1)}
            print(json.dumps(row), flush=True)
            del q, k, v, cache


if __name__ == "__main__":
    main()
