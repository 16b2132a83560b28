"""MoEMLP forward at Mixtral-8x7B widths (h 4096, f 14336, E 8, top-2, bf16,
eval): the fused ops.moe_ffn path against the per-expert library loop, by
token count. Device events around `iters` forwards over 8 rotating inputs
(so the routing varies), the two paths alternated `rounds` times; the median
round and the spread are printed, one JSON line per T.

  python tools/moe_ffn_bench.py [--iters 200] [--rounds 3]
  rocprofv3 --kernel-trace --stats -- python tools/moe_ffn_bench.py --trace T

--trace T runs 40 fused forwards at T tokens and prints the number of live
experts of each input, from which the bytes the two streaming kernels had to
read follow (gate/up: live * 2 * f * h * 2 B, down: live * h * f * 2 B)."""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from hypha_amd.models.moe import PRESETS, MoEMLP

DEV = torch.device("cuda", 0)
N_INPUTS = 8


def build():
    from dataclasses import replace

    cfg = replace(PRESETS["mixtral-8x7b"])
    torch.manual_seed(0)
    with torch.device("meta"):
        mlp = MoEMLP(cfg)
    mlp = mlp.bfloat16().to_empty(device=DEV).eval()
    for p in mlp.parameters():
        p.data.normal_(std=0.02)
    return mlp


def inputs(t):
    g = torch.Generator(device=DEV).manual_seed(100 + t)
    return [torch.randn(1, t, 4096, device=DEV, generator=g).bfloat16()
            for _ in range(N_INPUTS)]


@torch.no_grad()
def time_us(mlp, xs, fused, iters):
    mlp.cfg.fused_ffn_max_tokens = (1 << 30) if fused else 0
    for x in xs:
        mlp(x)
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    torch.cuda.synchronize()
    start.record()
    for i in range(iters):
        mlp(xs[i % N_INPUTS])
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace", type=int, default=0)
    args = ap.parse_args()
    mlp = build()
    if args.trace:
        xs = inputs(args.trace)
        with torch.no_grad():
            live = [len(set(mlp.router(x[0]).float().topk(2, -1).indices.reshape(-1).tolist()))
                    for x in xs]
            print(f"T={args.trace} live experts per input {live} mean {sum(live) / N_INPUTS}")
            mlp.cfg.fused_ffn_max_tokens = 1 << 30
            for i in range(40):
                mlp(xs[i % N_INPUTS])
        torch.cuda.synchronize()
        return
    for t in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512):
        xs = inputs(t)
        fused, loop = [], []
        for _ in range(args.rounds):
            fused.append(time_us(mlp, xs, True, args.iters))
            loop.append(time_us(mlp, xs, False, args.iters))
        med = lambda v: sorted(v)[len(v) // 2]
        print(json.dumps({"T": t, "fused_us": round(med(fused), 1),
                          "loop_us": round(med(loop), 1),
                          "fused_min_max": [round(min(fused), 1), round(max(fused), 1)],
                          "loop_min_max": [round(min(loop), 1), round(max(loop), 1)]}),
              flush=True)


main()
