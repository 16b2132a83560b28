"""Decode (serving) throughput microbench: prefill once, then timed
single-token KV-cache decode steps. Prints decode tokens/s."""

import argparse
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

# pre-tuned hipBLASLt algos (shared table with bench.py; includes the
# skinny decode shapes)
_TUNED_BASE = str(Path(__file__).resolve().parent.parent /
                  "tunableop_gfx950_llama8b.csv")
if (os.path.exists(_TUNED_BASE.replace(".csv", "0.csv"))
        and "PYTORCH_TUNABLEOP_ENABLED" not in os.environ):
    os.environ["PYTORCH_TUNABLEOP_ENABLED"] = "1"
    os.environ["PYTORCH_TUNABLEOP_TUNING"] = "0"
    os.environ["PYTORCH_TUNABLEOP_FILENAME"] = _TUNED_BASE

import torch


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="llama3-8b")
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--prefill", type=int, default=512)
    p.add_argument("--decode", type=int, default=128)
    p.add_argument("--warmup", type=int, default=16)
    p.add_argument("--graph", action="store_true",
                   help="hipGraph-captured decode step")
    p.add_argument("--sample", metavar="T[:K[:P]]", default=None,
                   help="sample with temperature T, top-k K (0 = off) and "
                        "top-p P. With --graph: the graphed decoder's sampling "
                        "graph (ops.sample_token, Philox uniforms). Without: "
                        "the eager loop, torch.multinomial unless P is given "
                        "(top-p needs sampler='philox')")
    p.add_argument("--kv-fp8", action="store_true",
                   help="fp8 (e4m3 + per-row scales) KV cache")
    p.add_argument("--ragged", metavar="LO:HI", default=None,
                   help="right-padded batch: prompt lengths drawn uniformly "
                        "from [LO, HI] (fixed seed, HI <= --prefill), generated "
                        "through the per-sequence-length path; LO == HI runs a "
                        "uniform batch through that path")
    p.add_argument("--paged", action="store_true",
                   help="paged KV cache (64-row pages, block table) in the "
                        "graphed decoder; needs --graph --ragged LO:HI. Prints "
                        "the KV bytes either layout allocates for the batch drawn")
    args = p.parse_args()
    if args.paged and not (args.graph and args.ragged is not None):
        raise SystemExit("--paged needs --graph --ragged LO:HI")

    from hypha_amd import models

    dev = "cuda:0"
    torch.manual_seed(0)
    with torch.device(dev):
        torch.set_default_dtype(torch.bfloat16)
        model = models.build(args.model)
        torch.set_default_dtype(torch.float32)
    model = model.to(dev).bfloat16().eval()
    for buf in model.buffers():  # rope tables must stay fp32 for the kernels
        if buf.dtype in (torch.bfloat16, torch.float16):
            buf.data = buf.data.float()
    ids = torch.randint(0, model.cfg.vocab_size - 1, (args.batch, args.prefill),
                        device=dev)

    kvq = "fp8" if args.kv_fp8 else None
    lens = None
    if args.ragged is not None:
        lo, hi = (int(x) for x in args.ragged.split(":"))
        if not 1 <= lo <= hi <= args.prefill:
            raise SystemExit(f"--ragged {args.ragged}: need 1 <= LO <= HI <= --prefill")
        g = torch.Generator().manual_seed(0)
        lens = torch.randint(lo, hi + 1, (args.batch,), generator=g)
    kv_note = ""
    if args.graph:
        from hypha_amd.runtime.graphed_decode import GraphedDecoder

        layout = {}
        if args.paged:
            from hypha_amd.models.paged_kv import PAGE, kv_bytes, pages_for

            # a count from shapes: the pool holds exactly the pages the drawn
            # batch needs; the contiguous slab charges every sequence
            # --prefill + new rows
            new = args.decode + args.warmup
            n_pages = sum(pages_for(n + new) for n in lens.tolist())
            layout = dict(kv_layout="paged", kv_pages=n_pages)
            cfg = model.cfg
            shape = (cfg.n_layers, cfg.n_kv_heads, cfg.head_dim, kvq)
            paged_b = kv_bytes(n_pages * PAGE, *shape)
            dense_b = kv_bytes(args.batch * (args.prefill + new), *shape)
            kv_note = (f"  [KV bytes: paged {paged_b} ({n_pages} pages), contiguous "
                       f"{dense_b}, ratio {paged_b / dense_b:.3f}]")
        dec = GraphedDecoder(model, args.batch, args.prefill,
                             args.decode + args.warmup, kv_quant=kvq, **layout)
        gen = dec.generate
    else:
        import functools

        gen = functools.partial(model.generate, kv_quant=kvq)

    tag = ""
    if args.sample is not None:
        import functools

        parts = args.sample.split(":")
        if not 1 <= len(parts) <= 3:
            raise SystemExit(f"--sample {args.sample}: expected T[:K[:P]]")
        kw = dict(temperature=float(parts[0]), seed=0,
                  top_k=int(parts[1]) if len(parts) > 1 else 0)
        if len(parts) > 2:
            kw["top_p"] = float(parts[2])
            if not args.graph:
                kw["sampler"] = "philox"
        gen = functools.partial(gen, **kw)
        tag = f" sample {args.sample}"
    if args.ragged is not None:
        import functools

        gen = functools.partial(gen, prompt_lens=lens)
        tag += " paged" if args.paged else ""
        tag += (f" ragged {lo}:{hi} (mean {lens.float().mean().item():.0f}, "
               f"max {int(lens.max())})")

    # warm (weights/algos/graph capture), then difference two WARM runs so
    # one-time costs never land in the per-token figure
    gen(ids, max_new_tokens=args.warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gen(ids, max_new_tokens=args.warmup)
    torch.cuda.synchronize()
    t_short = time.perf_counter() - t0
    t0 = time.perf_counter()
    out = gen(ids, max_new_tokens=args.decode + args.warmup)
    torch.cuda.synchronize()
    t_long = time.perf_counter() - t0
    dt = t_long - t_short
    toks = args.batch * args.decode
    if args.ragged is not None:
        out, out_lens = out
        assert out_lens.tolist() == (lens + args.decode + args.warmup).tolist()
    print(f"{args.model} b{args.batch} prefill{args.prefill}{tag}: "
          f"{toks / dt:.0f} decode tok/s  ({dt / args.decode * 1e3:.2f} ms/step)"
          f"  [prefill+{args.warmup}: {t_short:.2f}s]{kv_note}")
    assert out.shape[1] == args.prefill + args.decode + args.warmup


if __name__ == "__main__":
    main()
