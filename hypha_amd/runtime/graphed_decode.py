"""hipGraph-captured decoding (greedy or sampled) for the Llama family.

Eager single-token decode is LAUNCH-bound (measured 6.6 ms/step at b8 for
Llama-3-8B: ~300 kernels x ~4-6 us of launch+epilogue overhead each, while
the GEMMs themselves need ~2 ms of HBM time). The whole per-token step —
embed, per-layer norm/projections/RoPE/cache-append/decode-attention/MLP,
final norm, logits, token choice, bookkeeping — is captured ONCE as a hipGraph
and replayed per token with zero host round-trips:

* the cache length lives in a device int32 read by the decode kernel at
  kernel time (ops/hip/decode.hip attn_decode_graph), so one capture
  serves every step as the cache grows;
* RoPE rows are gathered with a device position index; the cache append is
  index_copy_ with the same index; the sampled token is written back into
  the graph's own input buffer, so replays chain with no synchronization.

Ragged batches (prompt_lens) and stop tokens (eos_token_id) run a SECOND,
lazily captured graph: the per-sequence cache lengths, the alive mask and the
stop/pad ids are device state, every position-dependent op takes them per
sequence (ops.apply_rope_qk_at, KVCache.append_rows, ops.attn_decode_varlen),
and a finished sequence parks its append out of range and attends over zero
rows. The uniform graph above is not touched by it.

Sampling (temperature > 0) has its own two lazily captured graphs, uniform
and ragged; the greedy graphs are not touched by them. Everything a draw
depends on is device state read at kernel time — Philox seed and step counter,
temperature, top_k, top_p — so one capture serves every seed and setting:
a step draws u = ops.philox_uniform(seed, step, B), picks with
ops.sample_token (ops/hip/sample.hip), records u in u_log[:, step] and
advances the counter inside the graph. The tokens are those of
model.generate(sampler="philox") with the same seed and parameters.

kv_layout="paged" keeps the cache in a pool of 64-row pages
(models/paged_kv.py). A paged decoder serves EVERY call through the two ragged
graphs (a uniform call is a ragged one with full lengths): the block table is
static device state, refilled on the host before a call's first step with the
pages of the whole call, so nothing is allocated inside a graph and a captured
graph stays valid across calls.
"""

from __future__ import annotations

import torch

from hypha_amd import ops
from hypha_amd.models.kv_cache import KVCache
from hypha_amd.models.llama import RaggedStep, check_prompt_lens, prefill_ragged
from hypha_amd.models.paged_kv import PagedKVCache, PageTable, pages_for


class GraphedDecoder:
    def __init__(self, model, batch: int, prompt_len: int, max_new: int,
                 kv_quant: str | None = None, kv_layout: str = "contiguous",
                 kv_pages: int | None = None, kv_free_order=None):
        from hypha_amd import _C

        if kv_layout not in ("contiguous", "paged"):
            raise ValueError(f"kv_layout must be 'contiguous' or 'paged', got {kv_layout!r}")

        self._C = _C
        self.model = model
        cfg = model.cfg
        dev = next(model.parameters()).device
        self.dev = dev
        self.batch = batch
        self.max_new = max_new
        self.kv_quant = kv_quant
        t_alloc = prompt_len + max_new
        self.kv_layout = kv_layout
        self.table = None
        if kv_layout == "paged":
            max_pages = pages_for(t_alloc)
            self.table = PageTable(batch, max_pages,
                                   batch * max_pages if kv_pages is None else kv_pages,
                                   dev, free_order=kv_free_order)
            self.caches = [PagedKVCache(self.table, cfg.n_kv_heads, cfg.head_dim,
                                        dev, dtype=next(model.parameters()).dtype,
                                        quant=kv_quant)
                           for _ in model.blocks]
        else:
            self.caches = [KVCache(batch, t_alloc, cfg.n_kv_heads, cfg.head_dim,
                                   dev, dtype=next(model.parameters()).dtype,
                                   quant=kv_quant)
                           for _ in model.blocks]
        # where a finished sequence's append goes (nothing is written there),
        # and the bound that sizes the decode kernel's split grid
        self.park = self.table.max_rows if self.table is not None else t_alloc
        self.tok = torch.zeros(batch, 1, dtype=torch.long, device=dev)
        self.pos = torch.zeros(1, dtype=torch.long, device=dev)
        self.t32 = torch.zeros(1, dtype=torch.int32, device=dev)
        self.step = torch.zeros(1, dtype=torch.long, device=dev)
        self.out = torch.zeros(batch, max_new, dtype=torch.long, device=dev)
        self.graph = None
        # ragged / stop-token state (second graph, captured on first use)
        self.t_alloc = t_alloc
        self.n_cache = torch.zeros(batch, dtype=torch.long, device=dev)
        self.alive = torch.ones(batch, dtype=torch.bool, device=dev)
        self.lens_out = torch.zeros(batch, dtype=torch.long, device=dev)
        self.tokens_r = torch.zeros(batch, t_alloc, dtype=torch.long, device=dev)
        self.eos_t = torch.full((1,), -1, dtype=torch.long, device=dev)  # -1: none
        self.pad_t = torch.zeros(1, dtype=torch.long, device=dev)
        self.graph_r = None
        # sampling state (third and fourth graph, captured on first use)
        self.s_seed = torch.zeros(1, dtype=torch.long, device=dev)
        self.s_step = torch.zeros(1, dtype=torch.long, device=dev)
        self.s_temp = torch.ones(1, dtype=torch.float32, device=dev)
        self.s_topk = torch.zeros(1, dtype=torch.int32, device=dev)
        self.s_topp = torch.ones(1, dtype=torch.float32, device=dev)
        self.u_log = torch.zeros(batch, max_new, dtype=torch.float32, device=dev)
        self.graph_s = None
        self.graph_rs = None

    def _pick(self, logits, sample: bool):
        """Next token [b, 1] from logits [b, V] (graph-capturable). Sampling
        draws this step's uniforms from the device seed/step, logs them and
        advances the step counter."""
        if not sample:
            return logits.argmax(-1, keepdim=True)
        u = ops.philox_uniform(self.s_seed, self.s_step, self.batch)
        nxt = ops.sample_token(logits, u, self.s_temp, self.s_topk, self.s_topp)
        self.u_log.index_copy_(1, self.s_step.clamp(max=self.max_new - 1), u[:, None])
        self.s_step += 1
        return nxt

    def _step(self, sample: bool = False) -> None:
        """One decode step over static device state (graph-capturable).
        GEMMs run 2-D through hipBLASLt (the hand-written skinny-M GEMV,
        ops/hip/skinny_gemm.hip, measured 0.4 TB/s vs the library's 1.8-5.9
        on these shapes — shuffle-reduction issue-bound; kept as an opt-in
        negative result like grouped_gemm)."""
        m = self.model
        cfg = m.cfg
        b = self.batch
        lin = lambda t, wt: t @ wt.t()  # noqa: E731
        x = m.embed(self.tok)
        cos = m.rope_cos.index_select(0, self.pos)
        sin = m.rope_sin.index_select(0, self.pos)
        for blk, cache in zip(m.blocks, self.caches):
            n1 = blk.attn_norm(x)[:, 0]  # [b, h]
            a = blk.attn
            q = lin(n1, a.wq.weight).view(b, 1, cfg.n_heads, cfg.head_dim)
            k = lin(n1, a.wk.weight).view(b, 1, cfg.n_kv_heads, cfg.head_dim)
            v = lin(n1, a.wv.weight).view(b, 1, cfg.n_kv_heads, cfg.head_dim)
            q, k = ops.apply_rope_qk(q, k, cos, sin, layout="bshd")
            cache.append_at(k, v, self.pos)
            if self.kv_quant == "fp8":
                o = self._C.attn_decode_fp8_graph(
                    q[:, 0].contiguous(), cache.k, cache.v, cache.k_scale,
                    cache.v_scale, self.t32)
            else:
                o = self._C.attn_decode_graph(q[:, 0].contiguous(), cache.k,
                                              cache.v, self.t32)
            attn_out = lin(o.reshape(b, -1), a.wo.weight).view(b, 1, -1)
            x, n2 = ops.add_rmsnorm(x, attn_out, blk.mlp_norm.weight,
                                    blk.mlp_norm.eps)
            n2f = n2[:, 0]
            h = ops.swiglu(lin(n2f, blk.mlp.w_gate.weight),
                           lin(n2f, blk.mlp.w_up.weight))
            x = x + lin(h, blk.mlp.w_down.weight).view(b, 1, -1)
        x = m.norm(x)
        head_w = m.lm_head.weight if m.lm_head is not None else m.embed.weight
        logits = lin(x[:, 0], head_w)
        nxt = self._pick(logits, sample)  # [b, 1]
        self.step.clamp_(max=self.max_new - 1)
        self.out.index_copy_(1, self.step, nxt)
        self.tok.copy_(nxt)
        self.pos += 1
        self.t32 += 1
        self.step += 1

    def _emit(self, x, sample: bool = False) -> None:
        """Ragged bookkeeping after a forward (graph-capturable): sample from
        hidden rows x [b, 1, h], write each live sequence's token directly
        after what it has, freeze the ones that emitted the stop token, and
        set the next input token."""
        m = self.model
        x = m.norm(x)
        head_w = m.lm_head.weight if m.lm_head is not None else m.embed.weight
        nxt = self._pick(x[:, 0] @ head_w.t(), sample)  # [b, 1]
        live = self.alive[:, None]
        at = self.n_cache.clamp(max=self.t_alloc - 1)[:, None]
        self.tokens_r.scatter_(1, at, torch.where(live, nxt, self.tokens_r.gather(1, at)))
        self.lens_out.copy_(torch.where(self.alive, self.n_cache + 1, self.lens_out))
        self.alive.logical_and_(nxt[:, 0] != self.eos_t)
        self.tok.copy_(torch.where(self.alive[:, None], nxt, self.pad_t.expand_as(nxt)))

    def _step_ragged(self, sample: bool = False) -> None:
        """One ragged decode step over static device state (graph-capturable):
        sequence b's current token sits at position n_cache[b]."""
        m = self.model
        step = RaggedStep(self.n_cache, self.alive, self.park, m.rope_cos.shape[0],
                          max_len=self.t_alloc)
        x = m.embed(self.tok)
        for blk, cache in zip(m.blocks, self.caches):
            x = blk(x, m.rope_cos, m.rope_sin, cache=cache, ragged=step)
        self.n_cache += self.alive.to(torch.long)
        self._emit(x, sample)

    def _generate_ragged(self, input_ids, max_new_tokens, prefill_chunk,
                         prompt_lens, eos_token_id, pad_token_id, sample=False):
        m = self.model
        b, s = input_ids.shape
        if s + max_new_tokens > self.t_alloc:
            raise ValueError(f"{s} + {max_new_tokens} tokens exceed the decoder's "
                             f"cache of {self.t_alloc} rows")
        lens = check_prompt_lens([s] * b if prompt_lens is None else prompt_lens,
                                 b, s, self.dev)
        total = s + max_new_tokens
        if self.table is not None and max_new_tokens > 0:
            # the pages of the whole call, before any step runs
            self.table.reserve((lens + max_new_tokens).tolist())
        self.tokens_r.fill_(pad_token_id)
        in_prompt = torch.arange(s, device=self.dev)[None, :] < lens[:, None]
        self.tokens_r[:, :s] = torch.where(in_prompt, input_ids, self.tokens_r[:, :s])
        self.n_cache.copy_(lens)
        self.lens_out.copy_(lens)
        self.alive.fill_(True)
        self.eos_t.fill_(-1 if eos_token_id is None else eos_token_id)
        self.pad_t.fill_(pad_token_id)
        if max_new_tokens > 0:
            self._emit(prefill_ragged(m, self.caches, input_ids, lens, prefill_chunk),
                       sample)
        n_replay = max_new_tokens - 1
        graph = self.graph_rs if sample else self.graph_r
        if n_replay > 0 and graph is None:
            if max_new_tokens < 8:  # not worth capturing: run eagerly
                for _ in range(n_replay):
                    self._step_ragged(sample)
                n_replay = 0
            else:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    self._step_ragged(sample)
                    self._step_ragged(sample)
                torch.cuda.current_stream().wait_stream(side)
                n_replay -= 2
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    self._step_ragged(sample)  # recorded, not executed
                if sample:
                    self.graph_rs = graph
                else:
                    self.graph_r = graph
        for _ in range(max(0, n_replay)):
            graph.replay()
        tokens = self.tokens_r[:, :total].clone()
        return (tokens, self.lens_out.clone()) if prompt_lens is not None else tokens

    @torch.no_grad()
    def generate(self, input_ids: torch.Tensor, max_new_tokens: int,
                 prefill_chunk: int | None = None, prompt_lens=None,
                 eos_token_id: int | None = None, pad_token_id: int = 0,
                 temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0,
                 seed: int | None = None):
        """prompt_lens / eos_token_id / pad_token_id as in
        LlamaForCausalLM.generate: with prompt_lens the batch is right-padded
        and the call returns (tokens, lens). The ragged path always runs
        max_new_tokens steps (no host round trip to see that all finished).

        temperature <= 0 decodes greedily. temperature > 0 samples as
        model.generate(sampler="philox") does (needs seed; top_k 0 = off,
        top_p in (0, 1]); u_log[:, i] then holds the uniforms of the i-th new
        token. A finished ragged sequence still draws but stays parked."""
        m = self.model
        b, s = input_ids.shape
        assert b == self.batch and max_new_tokens <= self.max_new
        if prefill_chunk is not None and prefill_chunk < 1:
            raise ValueError(f"prefill_chunk must be >= 1, got {prefill_chunk}")
        sample = temperature > 0
        if sample:
            if seed is None:
                raise ValueError("sampling (temperature > 0) needs a seed")
            ops.reference.check_sampling_params(temperature, top_k, top_p)
            self.s_seed.fill_(seed)
            self.s_step.zero_()
            self.s_temp.fill_(temperature)
            self.s_topk.fill_(min(int(top_k), 2 ** 31 - 1))
            self.s_topp.fill_(top_p)
            self.u_log.zero_()
        if self.table is not None:
            m.eval()
            return self._generate_ragged(input_ids, max_new_tokens, prefill_chunk,
                                         prompt_lens, eos_token_id, pad_token_id,
                                         sample)
        if prompt_lens is not None or eos_token_id is not None:
            m.eval()
            for cache in self.caches:
                cache.t = 0
            return self._generate_ragged(input_ids, max_new_tokens, prefill_chunk,
                                         prompt_lens, eos_token_id, pad_token_id,
                                         sample)
        m.eval()
        for cache in self.caches:  # reuse across generate() calls
            cache.t = 0
        # ---- prefill (eager; MFMA flash kernel for an aligned single pass,
        # the cache-reading prefill kernel for ragged or chunked prompts) ----
        step = s if prefill_chunk is None else prefill_chunk
        for p0 in range(0, s, step):
            x = m.embed(input_ids[:, p0:p0 + step])
            for blk, cache in zip(m.blocks, self.caches):
                x = blk(x, m.rope_cos, m.rope_sin, cache=cache, pos=p0)
        xl = m.norm(x[:, -1:])
        logits = (m.lm_head(xl) if m.lm_head is not None
                  else torch.nn.functional.linear(xl, m.embed.weight))
        g0 = self._pick(logits[:, 0], sample)
        self.out[:, 0:1].copy_(g0)
        self.tok.copy_(g0)
        self.pos.fill_(s)
        self.t32.fill_(s + 1)
        self.step.fill_(1)

        n_replay = max_new_tokens - 1
        graph = self.graph_s if sample else self.graph
        if n_replay > 0 and graph is None:
            if max_new_tokens < 8:  # not worth capturing: run eagerly
                for _ in range(n_replay):
                    self._step(sample)
                return torch.cat([input_ids, self.out[:, :max_new_tokens]], dim=1)
            # 2 warmup steps on a side stream (they are REAL steps), capture
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._step(sample)
                self._step(sample)
            torch.cuda.current_stream().wait_stream(side)
            n_replay -= 2
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self._step(sample)  # recorded, not executed
            if sample:
                self.graph_s = graph
            else:
                self.graph = graph
        for _ in range(max(0, n_replay)):
            graph.replay()
        return torch.cat([input_ids, self.out[:, :max_new_tokens]], dim=1)
