"""ops.linear_mxfp4w per shape: the weight-only MXFP4 kernel (ops/hip/
linear_mxfp4w.hip) against ops.linear_fp8w on e4m3 weights and x @ w_bf16.t()
on hipBLASLt, at Llama-3-8B's linear shapes and decode-sized M. On the gate/up
shape the op's own fallback (dequantise the codes to bf16, then the library)
is timed too: the largest M at which the kernel is not slower than it is the
max_rows default.

The method is tools/linear_fp8w_bench.py's: device events around a window of
at least --window seconds per contender (sized from a short calibration run),
contenders alternated --rounds times in one process, median round printed with
min and max; --graph times replays of a captured pass over the ring. Every
contender walks a ring of weight copies whose MXFP4 form is at least 512 MiB
in total (at most 64 copies), so that weights come from HBM. One JSON line per
(shape, M): times in us, weight bytes (for MXFP4 codes plus scales) over time
in TB/s, and the share of the peak HBM bandwidth (8 TB/s).

--act mxfp8 adds the MXFP8-activation mode (act_quant="mxfp8"): "a8" is the
whole op, quantise launch included, at the default prefetch depth; "a8_d1" and
"a8_d2" are the same through the binding at depths 1 and 2; "quant" is the
quantise launch alone, so a8 - quant is the GEMM (and reduce). a8_over_mxfp4w
is the ratio of the times per round: median, min and max.

  python tools/linear_mxfp4w_bench.py [--graph] [--window 0.5] [--rounds 3] [--ms 1,8,32]
                                      [--act mxfp8]
"""
import argparse
import json
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

# pre-tuned hipBLASLt algos, loaded as tools/decode_bench.py loads them
_TUNED_BASE = str(Path(__file__).resolve().parent.parent /
                  "tunableop_gfx950_llama8b.csv")
if (os.path.exists(_TUNED_BASE.replace(".csv", "0.csv"))
        and "PYTORCH_TUNABLEOP_ENABLED" not in os.environ):
    os.environ["PYTORCH_TUNABLEOP_ENABLED"] = "1"
    os.environ["PYTORCH_TUNABLEOP_TUNING"] = "0"
    os.environ["PYTORCH_TUNABLEOP_FILENAME"] = _TUNED_BASE

import torch

from hypha_amd import ops

DEV = torch.device("cuda", 0)
PEAK_HBM = 8.0e12  # bytes/s
RING_BYTES = 1 << 29
SHAPES = {  # name -> (N, K)
    "wq/wo": (4096, 4096),
    "wk/wv": (1024, 4096),
    "gate/up": (14336, 4096),
    "down": (4096, 14336),
    "head": (128256, 4096),
}


def ring(n, k):
    """Weight copies as (codes, scales, w8, scale, w_bf16)."""
    copies = max(1, min(64, -(-RING_BYTES // (n * k // 2))))
    g = torch.Generator(device=DEV).manual_seed(n + k)
    out = []
    for _ in range(copies):
        w = torch.randn(n, k, device=DEV, generator=g) / k ** 0.5
        out.append((*ops.quantize_mxfp4(w), *ops.quantize_rows_e4m3(w), w.bfloat16()))
    return out


def window_us(fn, n_ring, seconds, graph):
    """Mean time of fn(i) in us over a window of at least `seconds`. With
    graph, one pass over the ring (at least 20 calls) is captured and the
    window replays it, so no host launch cost is in the figure."""
    per_pass = max(20, n_ring)

    def one_pass():
        for i in range(per_pass):
            fn(i % n_ring)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm every copy: code objects, library algorithms
        one_pass()
    torch.cuda.current_stream().wait_stream(side)
    if graph:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            one_pass()
        one_pass = g.replay

    def run(passes):
        start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        torch.cuda.synchronize()
        start.record()
        for _ in range(passes):
            one_pass()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) * 1e3 / (passes * per_pass)

    est = run(1)
    return run(int(seconds * 1e6 / (est * per_pass)) + 1)


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--ms", default="1,8,32,64,128")
    ap.add_argument("--graph", action="store_true",
                    help="time replays of a captured graph: kernel time without "
                         "host launch cost, as in the graphed decoder")
    ap.add_argument("--act", choices=["mxfp8"], default=None,
                    help="also time the MXFP8-activation mode (see above)")
    ap.add_argument("--no-baselines", action="store_true",
                    help="leave out the bf16 library and the fallback contenders")
    args = ap.parse_args()
    ops.native_available_or_raise()
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for name in args.shapes.split(","):
        n, k = SHAPES[name]
        ws = ring(n, k)
        nbytes = {"mxfp4w": n * k // 2 + n * k // 32, "fp8w": n * k, "bf16": 2 * n * k}
        for m in (int(v) for v in args.ms.split(",")):
            x = torch.randn(m, k, device=DEV).bfloat16()
            contenders = {
                "mxfp4w": lambda i: ops.linear_mxfp4w(x, ws[i][0], ws[i][1], max_rows=1 << 30),
                "fp8w": lambda i: ops.linear_fp8w(x, ws[i][2], ws[i][3], max_rows=1 << 30),
                "bf16": lambda i: x @ ws[i][4].t(),
            }
            if args.act:
                from hypha_amd import _C
                contenders["a8"] = lambda i: ops.linear_mxfp4w(
                    x, ws[i][0], ws[i][1], max_rows=1 << 30, act_quant="mxfp8")
                contenders["a8_d1"] = lambda i: _C.linear_mxfp4w_a8(x, ws[i][0], ws[i][1], 1)
                contenders["a8_d2"] = lambda i: _C.linear_mxfp4w_a8(x, ws[i][0], ws[i][1], 2)
                contenders["quant"] = lambda i: ops.quantize_mxfp8(x)
            if args.no_baselines:
                del contenders["bf16"]
            elif name == "gate/up":
                contenders["fallback"] = lambda i: ops.linear_mxfp4w(x, ws[i][0], ws[i][1],
                                                                     max_rows=0)
            t = {c: [] for c in contenders}
            for _ in range(args.rounds):
                for c, fn in contenders.items():
                    t[c].append(window_us(fn, len(ws), args.window, args.graph))
            row = {"shape": name, "N": n, "K": k, "M": m, "copies": len(ws),
                   "graph": args.graph}
            for c in contenders:
                row[c + "_us"] = round(med(t[c]), 2)
                row[c + "_min_max"] = [round(min(t[c]), 2), round(max(t[c]), 2)]
            if args.act:
                r = [a / b for a, b in zip(t["a8"], t["mxfp4w"])]
                row["a8_over_mxfp4w"] = [round(v, 3) for v in (med(r), min(r), max(r))]
                row["a8_TBps"] = round(nbytes["mxfp4w"] / med(t["a8"]) / 1e6, 3)
            for c, b in nbytes.items():
                if c not in contenders:
                    continue
                row[c + "_TBps"] = round(b / med(t[c]) / 1e6, 3)
            row["mxfp4w_share_of_peak_hbm"] = round(
                nbytes["mxfp4w"] / (med(t["mxfp4w"]) * 1e-6) / PEAK_HBM, 3)
            print(json.dumps(row), flush=True)
        del ws
        torch.cuda.empty_cache()


main()
