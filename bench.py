"""Flagship benchmark: Llama-3-8B DiLoCo H=100 training throughput (tokens/s).

Driver contract:
  python bench.py --gpus N --steps K --warmup W
is launched (for N>1) as one rank per GPU under torch.distributed.run; each
rank reads RANK/LOCAL_RANK/WORLD_SIZE from the env. One timed "step" = one
DiLoCo inner step (forward + backward + fused AdamW) on the per-GPU batch;
outer RCCL syncs fire at their natural cadence (every H inner steps, counted
across warmup + timed region) so a run with steps >= H measures them in-line.
A separately-timed outer sync is always reported (outer_sync_ms, bytes) so
short runs still quantify the sync cost. Rank 0 prints ONE JSON line.

A plain run does only that: set up, warm up, time K steps, print the line.
--dump-outputs DIR additionally saves the last timed step's results (loss.npy,
params.npy) so two builds can be compared output for output; model init and
data are seeded, so the same arguments give the same inputs on every run.
--full is where measurements that need runs of their own belong.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

os.environ.setdefault("PYTORCH_ALLOC_CONF", "expandable_segments:True")

# Pre-tuned hipBLASLt algorithm selections for the flagship shapes (generated
# once with PYTORCH_TUNABLEOP_TUNING=1 on an MI355X; +2% step time).
# torch inserts the device ordinal before .csv: rank N reads ...llama8b{N}.csv
_TUNED_BASE = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                           "tunableop_gfx950_llama8b.csv")
_TUNED = _TUNED_BASE.replace(".csv", "0.csv")
if os.path.exists(_TUNED) and "PYTORCH_TUNABLEOP_ENABLED" not in os.environ:
    os.environ["PYTORCH_TUNABLEOP_ENABLED"] = "1"
    os.environ["PYTORCH_TUNABLEOP_TUNING"] = "0"
    os.environ["PYTORCH_TUNABLEOP_FILENAME"] = _TUNED_BASE

import torch

# --dump-outputs: elements of the flat parameter buffer kept when it is larger
_DUMP_SAMPLE = 1 << 22  # 4 Mi float32 = 16 MiB on disk


def dump_outputs(out_dir: str, worker, flat: torch.Tensor) -> None:
    """Write what a caller of the timed path holds after the last timed step:
    the loss train_step() returned and the parameters it updated in place.
    Parameters are read from the flat working buffer the model's tensors
    alias; a buffer over _DUMP_SAMPLE elements is reduced to a fixed, seeded
    index sample (same indices for the same model on every run)."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "loss.npy"),
            np.asarray([worker.last_loss], dtype=np.float64))
    n = flat.numel()
    if n > _DUMP_SAMPLE:
        g = torch.Generator(device="cpu").manual_seed(20240229)
        idx = torch.randint(0, n, (_DUMP_SAMPLE,), generator=g).sort().values
        vals = flat[idx.to(flat.device)]
    else:
        vals = flat
    np.save(os.path.join(out_dir, "params.npy"),
            vals.detach().float().cpu().numpy())


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--model", type=str, default="llama3-8b")
    p.add_argument("--batch", type=int, default=8, help="per-GPU batch (sequences)")
    p.add_argument("--seq-len", type=int, default=2048)
    p.add_argument("--h", type=int, default=100, help="DiLoCo inner steps per outer sync")
    p.add_argument("--device", type=str, default=None)
    p.add_argument("--fp8", action="store_true", help="fp8 e4m3 GEMMs (config 5 path)")
    p.add_argument("--fp8-weights", action="store_true",
                   help="fp8 WEIGHT STORAGE + fp8 GEMMs in the lean engine (config 5)")
    p.add_argument("--expert-parallel", action="store_true",
                   help="shard MoE experts across ranks (RCCL all-to-all per step; "
                        "outer sync covers shared params only)")
    p.add_argument("--state-bits", type=int, default=32, choices=(32, 8))
    p.add_argument("--grad-checkpoint", action="store_true",
                   help="per-block activation checkpointing (70B-class fits)")
    p.add_argument("--memory-mode", default="full", choices=("full", "lean"),
                   help="lean: bf16-SR master-free params, 8-bit state, streamed "
                        "grads, host theta0 (configs 4/5 sizing)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last timed step "
                        "produced (loss + a fixed seeded sample of the updated "
                        "parameters) as DIR/<name>.npy")
    p.add_argument("--full", action="store_true",
                   help="also run the secondary measurements that need runs of "
                        "their own (none at present: every figure in the result "
                        "line is a by-product of the plain run)")
    args = p.parse_args()

    from hypha_amd import models, ops
    from hypha_amd.data.synthetic import SyntheticTokens
    from hypha_amd.parallel import Comm, DiLoCoConfig, DiLoCoWorker, InnerOptConfig

    comm = Comm()
    n_gpus = comm.world_size if comm.is_distributed else args.gpus
    rank = comm.rank

    on_gpu = torch.cuda.is_available() and args.device != "cpu"
    device = torch.device("cuda", comm.local_rank) if on_gpu else torch.device("cpu")
    if on_gpu:
        ops.native_available_or_raise()

    if args.fp8_weights and on_gpu:
        args.memory_mode = "lean"  # fp8 weight storage lives in the lean engine
    torch.manual_seed(1234)
    # build directly on the GPU: 8 ranks x 32 GB of fp32 CPU-side init would
    # strain host RAM and add ~a minute per rank; rank-0's broadcast makes
    # every rank's weights identical regardless of init device RNG
    import contextlib

    build_ctx = torch.device(device) if on_gpu else contextlib.nullcontext()
    if args.memory_mode == "lean":
        torch.set_default_dtype(torch.bfloat16)  # build 46B+ models without a
        # transient fp32 copy (187 GB for Mixtral); rope tables stay fp32
    with build_ctx:
        overrides = {}
        if args.grad_checkpoint:
            overrides["gradient_checkpointing"] = True
        try:
            model = models.build(args.model, **overrides)
        except TypeError:  # model family without the flag
            model = models.build(args.model)
    torch.set_default_dtype(torch.float32)
    if args.expert_parallel:
        from hypha_amd.models.moe import shard_experts_

        n_shard = shard_experts_(model, comm.rank, max(1, comm.world_size))
        if rank == 0:
            print(f"# expert-parallel: sharded {n_shard} MoE layers over "
                  f"{comm.world_size} ranks", file=sys.stderr)
    if args.fp8 and on_gpu:
        from hypha_amd.ops.fp8 import convert_linears_to_fp8

        n_conv = convert_linears_to_fp8(model)
        if rank == 0:
            print(f"# fp8: converted {n_conv} linears", file=sys.stderr)
    cfg = DiLoCoConfig(
        h=args.h,
        inner=InnerOptConfig(lr=4e-4, warmup_steps=10, schedule="constant",
                             state_bits=args.state_bits),
    )
    if args.memory_mode == "lean":
        from hypha_amd.parallel import LeanDiLoCoWorker

        worker = LeanDiLoCoWorker(model, cfg, comm=comm, device=device,
                                  fp8_weights=args.fp8_weights and on_gpu)
    else:
        worker = DiLoCoWorker(model, cfg, comm=comm, device=device)
    data = SyntheticTokens(
        model.cfg.vocab_size, args.seq_len, args.batch, seed=77, rank=rank
    )

    def sync():
        if on_gpu:
            torch.cuda.synchronize()
        comm.barrier()

    def one_step():
        ids, labels = data.next_batch()
        worker.train_step(ids, labels)
        worker.maybe_outer_sync()

    # ---- warmup (untimed) ----
    for _ in range(args.warmup):
        one_step()

    # measure one outer sync explicitly (outside the timed region)
    sync()
    t0 = time.perf_counter()
    worker.outer_sync()
    sync()
    outer_sync_s = time.perf_counter() - t0
    rounds_before = worker.round

    # Phase-shift the H cadence so at least one outer sync lands INSIDE the
    # driver-timed window even when steps < H (it fires after ~steps/2 timed
    # steps). The whole-run cadence is still one sync per H inner steps; a
    # short window therefore OVER-charges the sync cost in `value` (1/K
    # instead of 1/H of a sync per step) — the conservative side. The true
    # H-amortized figure is reported as amortized_tokens_per_sec.
    worker.steps_in_round = max(0, args.h - max(1, min(args.steps, args.h) // 2))

    # ---- timed region: exactly K steps ----
    sync()
    t_start = time.perf_counter()
    for _ in range(args.steps):
        one_step()
    sync()
    elapsed = time.perf_counter() - t_start
    elapsed = comm.all_reduce_scalar(elapsed, op="max")

    tokens_per_step_job = args.batch * args.seq_len * n_gpus
    value = tokens_per_step_job * args.steps / elapsed
    ms_per_step = elapsed / args.steps * 1000.0
    # pure step time with the in-window syncs backed out (for H-amortization)
    synced_now = worker.round - rounds_before
    step_s_ex_sync = max(1e-9, elapsed - synced_now * outer_sync_s) / args.steps

    model_numel = (worker.numel + getattr(worker, "fp8_numel", 0)
                   if args.memory_mode == "lean" else worker.fp.numel)
    payload_bytes_per_sync = model_numel * 2  # bf16 comm dtype
    synced_in_window = worker.round - rounds_before
    if args.dump_outputs and rank == 0 and args.steps > 0:
        dump_outputs(args.dump_outputs, worker,
                     worker.flat if args.memory_mode == "lean" else worker.fp.flat)
    if rank == 0:
        result = {
            "metric": "tokens/sec (node) + outer-sync bytes, Llama-3-8B DiLoCo H=100 at 1/2/4/8 GPUs",
            "value": value,
            "unit": "tokens/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": ("fp8-weights/fp8-gemm" if args.fp8_weights
                      else "fp8-gemm/bf16" if args.fp8 else "bf16")
                     if on_gpu else "fp32",
            "data": "synthetic",
            "config": {
                "model": args.model,
                "global_batch": args.batch * n_gpus,
                "seq_len": args.seq_len,
                "parallelism": (f"ep{n_gpus}+diloco" if args.expert_parallel
                                else f"diloco-dp{n_gpus}"),
                "h": args.h,
                "model_params": model_numel,
                "memory_mode": args.memory_mode,
                "outer_syncs_in_timed_window": synced_in_window,
                "outer_sync_payload_bytes": payload_bytes_per_sync,
                "outer_sync_wire_bytes_per_rank": comm.wire_bytes_per_rank(payload_bytes_per_sync),
                "outer_sync_ms": outer_sync_s * 1000.0,
                "amortized_tokens_per_sec": tokens_per_step_job
                / (step_s_ex_sync + outer_sync_s / args.h),
                "comm_reduction_vs_ddp": f"{args.h}x fewer syncs, bf16 payload",
                "native_ops": ops.has_native(),
                "last_loss": worker.last_loss,
            },
        }
        print(json.dumps(result), flush=True)
    comm.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
