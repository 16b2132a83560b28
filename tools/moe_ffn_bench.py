"""MoEMLP forward at Mixtral-8x7B widths (h 4096, f 14336, E 8, top-2, bf16,
eval): the fused ops.moe_ffn path against the per-expert library loop, by
token count. Device events around `iters` forwards over 8 rotating inputs
(so the routing varies), the two paths alternated `rounds` times; the median
round and the spread are printed, one JSON line per T.

  python tools/moe_ffn_bench.py [--iters 200] [--rounds 3] [--w-fp8 | --w-mxfp4 [--a-mxfp8]]
  rocprofv3 --kernel-trace --stats -- python tools/moe_ffn_bench.py --trace T [--w-fp8 | --w-mxfp4 [--a-mxfp8]]

--w-fp8 times three paths the same way: a copy of the module on weight-only
fp8 experts (MoEMLP.quantize_experts_fp8_) through ops.moe_ffn_fp8w and
through its fallback loop of ops.linear_fp8w, and the bf16 module's fused path
as the baseline for time.

--w-mxfp4 does the same for a copy on weight-only MXFP4 experts
(MoEMLP.quantize_experts_mxfp4_): ops.moe_ffn_mxfp4w, its fallback loop of
ops.linear_mxfp4w, and the fp8 and bf16 fused paths as baselines, all four
alternated in one call.

--a-mxfp8 (with --w-mxfp4) adds a second copy of the MXFP4 module with
act_quant="mxfp8" (MXFP8 activations, ops.moe_ffn_mxfp4w(..., act_quant="mxfp8"))
as a fifth path, alternated with the others.

--trace T runs 40 fused forwards at T tokens (on the fp8 experts with --w-fp8,
on the MXFP4 experts with --w-mxfp4, in their MXFP8 mode with --a-mxfp8)
and prints the number of live experts of each input, from which the bytes the
two streaming kernels had to read follow (gate/up: live * 2 * f * h * B, down:
live * h * f * B, B = 2 bytes per bf16 weight, 1 per fp8 code, 17 / 32 per
MXFP4 weight: half a byte of code and 1 / 32 of a scale byte)."""
import argparse
import copy
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from hypha_amd.models.moe import PRESETS, MoEMLP

DEV = torch.device("cuda", 0)
N_INPUTS = 8
LIMITS = ("fused_ffn_max_tokens", "fused_ffn_fp8_max_tokens", "fused_ffn_mxfp4_max_tokens")


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
    for name in LIMITS:
        setattr(mlp.cfg, name, (1 << 30) if fused else 0)
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
    ap.add_argument("--w-fp8", action="store_true")
    ap.add_argument("--w-mxfp4", action="store_true")
    ap.add_argument("--a-mxfp8", action="store_true")
    args = ap.parse_args()
    if args.a_mxfp8 and not args.w_mxfp4:
        ap.error("--a-mxfp8 needs --w-mxfp4")
    mlp = build()
    mlp8 = mlp4 = None
    if args.w_fp8 or (args.w_mxfp4 and not args.trace):
        mlp8 = copy.deepcopy(mlp)  # its own cfg object too
        mlp8.quantize_experts_fp8_()
    if args.w_mxfp4:
        mlp4 = copy.deepcopy(mlp)
        mlp4.quantize_experts_mxfp4_()
    if args.a_mxfp8:
        mlp4a = copy.deepcopy(mlp4)  # the same codes, the other numerical mode
        mlp4a.act_quant = "mxfp8"
    if args.trace:
        xs = inputs(args.trace)
        run = mlp4a if args.a_mxfp8 else mlp4 if args.w_mxfp4 else mlp8 if args.w_fp8 else mlp
        with torch.no_grad():
            live = [len(set(mlp.router(x[0]).float().topk(2, -1).indices.reshape(-1).tolist()))
                    for x in xs]
            print(f"T={args.trace} live experts per input {live} mean {sum(live) / N_INPUTS}")
            for name in LIMITS:
                setattr(run.cfg, name, 1 << 30)
            for i in range(40):
                run(xs[i % N_INPUTS])
        torch.cuda.synchronize()
        return
    # (result key, module, fused path?)
    paths = [("fused", mlp, True), ("loop", mlp, False)]
    if args.w_fp8:
        paths = [("fp8_fused", mlp8, True), ("fp8_loop", mlp8, False), ("bf16_fused", mlp, True)]
    if args.w_mxfp4:
        paths = [("mxfp4_fused", mlp4, True), ("mxfp4_loop", mlp4, False),
                 ("fp8_fused", mlp8, True), ("bf16_fused", mlp, True)]
    if args.a_mxfp8:
        paths.insert(1, ("mxfp4_a8_fused", mlp4a, True))
    token_counts = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512)
    if args.w_fp8 or args.w_mxfp4:  # the loops dequantise whole experts above 128 rows: look further
        token_counts += (1024, 2048, 4096)
    for t in token_counts:
        xs = inputs(t)
        times = {key: [] for key, _, _ in paths}
        for _ in range(args.rounds):
            for key, module, fused in paths:
                times[key].append(time_us(module, xs, fused, args.iters))
        med = lambda v: sorted(v)[len(v) // 2]
        row = {"T": t}
        for key, v in times.items():
            row[key + "_us"] = round(med(v), 1)
            row[key + "_min_max"] = [round(min(v), 1), round(max(v), 1)]
        if args.w_fp8 and not args.w_mxfp4:  # the rule that sets fused_ffn_fp8_max_tokens
            row["fp8_fused_wins_every_round"] = all(
                a < b for a, b in zip(times["fp8_fused"], times["fp8_loop"]))
        if args.w_mxfp4:  # the rule that sets fused_ffn_mxfp4_max_tokens
            row["mxfp4_fused_wins_every_round"] = all(
                a < b for a, b in zip(times["mxfp4_fused"], times["mxfp4_loop"]))
        print(json.dumps(row), flush=True)


main()
