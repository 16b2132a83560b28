"""Inference executor: serves generation jobs through the same job-bridge
contract as training ({SOCKET_PATH}/{WORK_DIR}/{JOB_JSON}).

The reference positions itself as orchestration "for AI training AND
inference" with inference delegated to the same executor mechanism; this
executor is the native counterpart: it fetches prompt slices via the bridge
(scheduler-tracked data slices), runs KV-cache generation on the model
registry, writes completions as SafeTensors to the work dir, pushes them to
the configured result peers, and reports per-batch Status/Metrics progress
so the scheduler's FSM and lease machinery apply unchanged.

Job config: {"model", "data": <fetch ref>, "results": <send ref>?,
             "max_new_tokens", "batch_size", "seq_len", "temperature",
             "top_k", "top_p"?, "sampler": "philox"?, "seed"?,
             "num_batches", "kv_cache": "fp8"?,
             "prefill_chunk": <int>?, "pad_token_id": <int>?,
             "eos_token_id": <int>?, "kv_layout": "paged"?, "kv_pages": <int>?}

Llama-family jobs on GPU decode through the hipGraph-captured step
(runtime/graphed_decode.py) when they are greedy, or when they sample with
"sampler": "philox" (temperature > 0; "top_k", "top_p" and "seed" apply: the
tokens are a function of the prompt, the seed and those parameters, drawn by
ops.sample_token from Philox uniforms). Without "sampler", a job with a
temperature samples with torch.multinomial on the eager path. "kv_cache": "fp8" halves KV memory;
"prefill_chunk" feeds each prompt in pieces of at most that many tokens
(activation memory bounded by the chunk; absent = one pass).

"pad_token_id" makes every batch RAGGED: prompts are right-padded rows, a
prompt's length is its row without the trailing run of that id (at least one
token is kept), each sequence continues directly after its own prompt, and
the completion file gains a "lens" tensor (final valid length per sequence)
next to "tokens". "eos_token_id" stops a sequence at that token.

"kv_layout": "paged" keeps the KV cache in a pool of 64-row pages
(models/paged_kv.py): a sequence is charged the pages of its own length
instead of the batch's longest. "kv_pages" sizes the pool (default: what the
batch shape can need at most in the graphed decoder, exactly what each batch
needs on the eager path); a batch that needs more fails with
PagePoolExhausted. The completions are those of the contiguous layout.
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import torch


def prompt_lengths(prompts: torch.Tensor, pad_token_id: int) -> torch.Tensor:
    """Length of each right-padded row [B, s] without its trailing run of
    pad_token_id; at least 1 (an all-pad row keeps its first token)."""
    s = prompts.shape[1]
    not_pad = prompts != pad_token_id
    last = torch.where(not_pad, torch.arange(1, s + 1, device=prompts.device), 0)
    return last.amax(dim=1).clamp(min=1)


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--socket", required=True)
    p.add_argument("--work-dir", required=True)
    p.add_argument("--job", required=True)
    args = p.parse_args()

    from safetensors.torch import save_file

    from hypha_amd import models
    from hypha_amd.data.synthetic import load_slice
    from hypha_amd.runtime.session import Session

    with open(args.job) as f:
        cfg = json.load(f)

    session = Session(args.socket)
    from hypha_amd.telemetry import get_tracer

    tracer = get_tracer()
    disp_ns = os.environ.get("HYPHA_DISPATCH_TS_NS")
    if disp_ns:
        d = tracer.start_span("job.dispatch",
                              job_id=os.environ.get("HYPHA_JOB_ID", ""))
        d.start_ns = int(disp_ns)
        d.end()
    job_span = tracer.start_span("job.execute", kind_attr="generate",
                                 job_id=os.environ.get("HYPHA_JOB_ID", ""))
    torch.manual_seed(int(cfg.get("seed", 0)))
    device = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    model = models.build(cfg["model"])
    model.to(device=device,
             dtype=torch.bfloat16 if device.type == "cuda" else torch.float32)
    for buf in model.buffers():
        if buf.dtype in (torch.bfloat16, torch.float16):
            buf.data = buf.data.float()
    model.eval()

    batch_size = int(cfg.get("batch_size", 1))
    seq_len = int(cfg.get("seq_len", 64))
    max_new = int(cfg.get("max_new_tokens", 32))
    num_batches = int(cfg.get("num_batches", 1))
    temperature = float(cfg.get("temperature", 0.0))
    top_k = int(cfg.get("top_k", 0))
    top_p = float(cfg.get("top_p", 1.0))
    sampler = cfg.get("sampler", "multinomial")
    philox = sampler == "philox" and temperature > 0
    sample_kw = {}
    if philox:
        sample_kw = dict(temperature=temperature, top_k=top_k, top_p=top_p,
                         seed=int(cfg.get("seed", 0)))
    elif sampler not in ("multinomial", "philox"):
        raise ValueError(f"unknown sampler {sampler!r}")
    elif sampler == "multinomial" and top_p != 1.0:
        raise ValueError('"top_p" needs "sampler": "philox"')
    prefill_chunk = cfg.get("prefill_chunk")
    if prefill_chunk is not None:
        prefill_chunk = int(prefill_chunk)
        if prefill_chunk < 1:
            raise ValueError(f"prefill_chunk must be >= 1, got {prefill_chunk}")
    kv_layout = cfg.get("kv_layout", "contiguous")
    if kv_layout not in ("contiguous", "paged"):
        raise ValueError(f"unknown kv_layout {kv_layout!r}")
    layout_kw = {}
    if kv_layout == "paged":
        layout_kw["kv_layout"] = "paged"
        if cfg.get("kv_pages") is not None:
            layout_kw["kv_pages"] = int(cfg["kv_pages"])
    pad_id = cfg.get("pad_token_id")
    eos_id = cfg.get("eos_token_id")
    ragged_kw = {}
    if eos_id is not None:
        ragged_kw["eos_token_id"] = int(eos_id)
    if pad_id is not None:
        ragged_kw["pad_token_id"] = int(pad_id)

    # Llama-family serving on GPU, greedy or Philox-sampled: hipGraph-captured
    # decode step (runtime/graphed_decode.py; eager decode is launch-bound)
    graphed = None
    if ((temperature <= 0 or philox) and device.type == "cuda"
            and type(model).__name__ == "LlamaForCausalLM"
            and model.cfg.head_dim in (64, 128)
            and model.cfg.n_heads // model.cfg.n_kv_heads <= 8):
        from hypha_amd.runtime.graphed_decode import GraphedDecoder

        graphed = GraphedDecoder(model, batch_size, seq_len, max_new,
                                 kv_quant=cfg.get("kv_cache"), **layout_kw)

    done_batches = 0
    out_idx = 0
    while done_batches < num_batches:
        got = session.fetch(cfg["data"])
        for path in got["files"]:
            ids = load_slice(path)
            for i in range(0, ids.shape[0] - batch_size + 1, batch_size):
                if done_batches >= num_batches:
                    break
                prompts = ids[i : i + batch_size, :seq_len].to(device)
                kw = dict(ragged_kw)
                if pad_id is not None:
                    kw["prompt_lens"] = prompt_lengths(prompts, int(pad_id))
                if graphed is not None and prompts.shape[0] == batch_size:
                    out = graphed.generate(prompts, max_new_tokens=max_new,
                                           prefill_chunk=prefill_chunk, **kw,
                                           **sample_kw)
                elif philox:
                    out = model.generate(prompts, max_new_tokens=max_new,
                                         prefill_chunk=prefill_chunk,
                                         sampler="philox", **kw, **sample_kw,
                                         **layout_kw)
                else:
                    out = model.generate(prompts, max_new_tokens=max_new,
                                         temperature=temperature, top_k=top_k,
                                         seed=0, prefill_chunk=prefill_chunk, **kw,
                                         **layout_kw)
                result = {}
                if pad_id is not None:
                    out, lens = out
                    result["lens"] = lens.cpu().contiguous()
                result["tokens"] = out.cpu().contiguous()
                fname = f"completion-{out_idx:05d}.safetensors"
                save_file(result,
                          os.path.join(args.work_dir, fname))
                out_idx += 1
                if cfg.get("results"):
                    session.send_resource(cfg["results"], fname)
                done_batches += 1
                session.send_status({"kind": "status", "batch_size": batch_size})
            if done_batches >= num_batches:
                break
    session.send_status(
        {"kind": "metrics", "round": 0,
         "metrics": {"completions": float(out_idx)}}
    )
    print(f"[infer] wrote {out_idx} completion batches", flush=True)
    job_span.set_attribute("completions", out_idx)
    job_span.end()
    tracer.flush()
    session.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
