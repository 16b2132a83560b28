"""Llama-3-family dense transformer, built on hypha_amd.ops.

From-scratch modules (no HF): RMSNorm + RoPE + GQA causal attention +
SwiGLU MLP + tied/untied LM head + fused CE loss. Mirrors the model
capability the reference reaches through HF Auto classes
(/root/reference/executors/accelerate/src/hypha/accelerate_executor/model.py),
but implemented directly so the hot ops are our CDNA4 HIP kernels.
"""

from __future__ import annotations

import math
from dataclasses import dataclass, field

import torch
import torch.nn as nn

from hypha_amd import ops


@dataclass
class LlamaConfig:
    vocab_size: int = 128256
    hidden_size: int = 4096
    n_layers: int = 32
    n_heads: int = 32
    n_kv_heads: int = 8
    ffn_hidden: int = 14336
    max_seq_len: int = 8192
    rope_base: float = 500000.0
    norm_eps: float = 1e-5
    tie_embeddings: bool = False
    gradient_checkpointing: bool = False
    init_std: float = 0.02
    extra: dict = field(default_factory=dict)

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.n_heads

    def num_params(self) -> int:
        h, v, f = self.hidden_size, self.vocab_size, self.ffn_hidden
        hd = self.head_dim
        attn = h * (self.n_heads * hd) + 2 * h * (self.n_kv_heads * hd) + (self.n_heads * hd) * h
        mlp = 3 * h * f
        per_layer = attn + mlp + 2 * h
        emb = v * h * (1 if self.tie_embeddings else 2)
        return per_layer * self.n_layers + emb + h


# Named presets (sizes per the public Llama-3 architecture; BASELINE.json configs)
PRESETS: dict[str, LlamaConfig] = {
    "llama3-8b": LlamaConfig(),
    "llama3-70b": LlamaConfig(
        hidden_size=8192, n_layers=80, n_heads=64, n_kv_heads=8, ffn_hidden=28672
    ),
    # small debug model for CPU tests
    "llama-tiny": LlamaConfig(
        vocab_size=512, hidden_size=128, n_layers=2, n_heads=2, n_kv_heads=2,
        ffn_hidden=256, max_seq_len=256, rope_base=10000.0,
    ),
    # ~124M GPT-2-small-scale llama-style model for the CPU plumbing config
    "gpt2-small": LlamaConfig(
        vocab_size=50304, hidden_size=768, n_layers=12, n_heads=12, n_kv_heads=12,
        ffn_hidden=2048, max_seq_len=1024, rope_base=10000.0, tie_embeddings=True,
    ),
}


class RMSNorm(nn.Module):
    def __init__(self, dim: int, eps: float):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.eps = eps

    def forward(self, x):
        return ops.rmsnorm(x, self.weight, self.eps)


class Attention(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.cfg = cfg
        hd = cfg.head_dim
        self.wq = nn.Linear(cfg.hidden_size, cfg.n_heads * hd, bias=False)
        self.wk = nn.Linear(cfg.hidden_size, cfg.n_kv_heads * hd, bias=False)
        self.wv = nn.Linear(cfg.hidden_size, cfg.n_kv_heads * hd, bias=False)
        self.wo = nn.Linear(cfg.n_heads * hd, cfg.hidden_size, bias=False)

    def forward(self, x, cos, sin, cache=None, pos: int = 0, seq_lens=None,
                ragged=None):
        b, s, _ = x.shape
        cfg = self.cfg
        hd = cfg.head_dim
        # BSHD layout throughout: the projections' natural layout, consumed
        # directly by the stride-aware RoPE/attention kernels (no transposes)
        q = self.wq(x).view(b, s, cfg.n_heads, hd)
        k = self.wk(x).view(b, s, cfg.n_kv_heads, hd)
        v = self.wv(x).view(b, s, cfg.n_kv_heads, hd)
        if cache is None:
            q, k = ops.apply_rope_qk(q, k, cos, sin, layout="bshd")
            o = ops.flash_attention(q, k, v, causal=True, layout="bshd")
            return self.wo(o.reshape(b, s, -1))
        # inference with KV cache: rotate at absolute positions, append into
        # the pre-allocated bshd cache, then attend over the valid prefix.
        # Decode (s==1) runs the native flash-decoding kernel; an aligned
        # first pass runs the MFMA flash kernel; ragged prompts and chunked
        # continuation run the cache-reading prefill kernel (ops.attn_prefill).
        if ragged is not None:
            # ragged decode step (s == 1): every sequence at its own position
            o = ragged.attend(q, k, v, cos, sin, cache)
            return self.wo(o.reshape(b, 1, -1))
        q, k = ops.apply_rope_qk(q, k, cos[pos:], sin[pos:], layout="bshd")
        if hasattr(cache, "table"):
            # paged cache (always the per-sequence route): only the rows a
            # sequence has are written, into its own pages
            cache.append_chunk(k, v, pos, seq_lens)
            o = ops.attn_prefill_paged(q, cache.k, cache.v, cache.table.table, pos,
                                       cache.k_scale, cache.v_scale,
                                       seq_lens=seq_lens)
            return self.wo(o.reshape(b, s, -1))
        t = cache.append(k, v)
        if seq_lens is not None:
            # right-padded batch: the pads' K/V rows are written like any
            # other (decode overwrites them); the kernel skips what a short
            # sequence does not have
            o = ops.attn_prefill(q, cache.k, cache.v, pos, cache.k_scale,
                                 cache.v_scale, seq_lens=seq_lens)
            return self.wo(o.reshape(b, s, -1))
        if s == 1:
            o = ops.attn_decode(q[:, 0].contiguous(), cache.k, cache.v, t,
                                cache.k_scale, cache.v_scale)
            return self.wo(o.reshape(b, 1, -1))
        if pos == 0 and (not x.is_cuda or s % 128 == 0):
            o = ops.flash_attention(q, k, v, causal=True, layout="bshd")
            return self.wo(o.reshape(b, s, -1))
        # ragged prompt or chunked continuation: attend over the cache
        o = ops.attn_prefill(q, cache.k, cache.v, pos, cache.k_scale,
                             cache.v_scale)
        return self.wo(o.reshape(b, s, -1))


class MLP(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.w_gate = nn.Linear(cfg.hidden_size, cfg.ffn_hidden, bias=False)
        self.w_up = nn.Linear(cfg.hidden_size, cfg.ffn_hidden, bias=False)
        self.w_down = nn.Linear(cfg.ffn_hidden, cfg.hidden_size, bias=False)

    def forward(self, x):
        return self.w_down(ops.swiglu(self.w_gate(x), self.w_up(x)))


class Block(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.attn_norm = RMSNorm(cfg.hidden_size, cfg.norm_eps)
        self.attn = Attention(cfg)
        self.mlp_norm = RMSNorm(cfg.hidden_size, cfg.norm_eps)
        self.mlp = MLP(cfg)

    def forward(self, x, cos, sin, cache=None, pos: int = 0, seq_lens=None,
                ragged=None):
        attn_out = self.attn(self.attn_norm(x), cos, sin, cache=cache, pos=pos,
                             seq_lens=seq_lens, ragged=ragged)
        # fused residual-add + norm: one kernel writes the residual stream
        # and the normalized MLP input (saves an elementwise pass per block)
        x, n2 = ops.add_rmsnorm(x, attn_out, self.mlp_norm.weight,
                                self.mlp_norm.eps)
        x = x + self.mlp(n2)
        return x

    def forward_pair(self, res, delta, cos, sin):
        """Training fast path with the residual add DEFERRED: receives the
        previous block's (residual, sub-block output) pair so EVERY residual
        add fuses into the next norm kernel (including across blocks)."""
        res, n1 = ops.add_rmsnorm(res, delta, self.attn_norm.weight,
                                  self.attn_norm.eps)
        attn_out = self.attn(n1, cos, sin)
        res, n2 = ops.add_rmsnorm(res, attn_out, self.mlp_norm.weight,
                                  self.mlp_norm.eps)
        return res, self.mlp(n2)


class LlamaForCausalLM(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.cfg = cfg
        self.embed = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        self.blocks = nn.ModuleList(Block(cfg) for _ in range(cfg.n_layers))
        self.norm = RMSNorm(cfg.hidden_size, cfg.norm_eps)
        if cfg.tie_embeddings:
            self.lm_head = None
        else:
            self.lm_head = nn.Linear(cfg.hidden_size, cfg.vocab_size, bias=False)
        cos, sin = ops.reference.rope_cos_sin(cfg.max_seq_len, cfg.head_dim, cfg.rope_base)
        self.register_buffer("rope_cos", cos, persistent=False)
        self.register_buffer("rope_sin", sin, persistent=False)
        self.apply(self._init)
        # scaled init on residual-out projections (GPT-2/Llama practice)
        for blk in self.blocks:
            for lin in (blk.attn.wo, blk.mlp.w_down):
                nn.init.normal_(lin.weight, std=cfg.init_std / math.sqrt(2 * cfg.n_layers))

    def _init(self, m):
        if isinstance(m, nn.Linear):
            nn.init.normal_(m.weight, std=self.cfg.init_std)
        elif isinstance(m, nn.Embedding):
            nn.init.normal_(m.weight, std=self.cfg.init_std)

    def forward(self, input_ids: torch.Tensor, labels: torch.Tensor | None = None):
        x = self.embed(input_ids)
        cos, sin = self.rope_cos, self.rope_sin
        # (residual, delta) carry: every residual add — including the
        # cross-block one — fuses into the next RMSNorm kernel; the final
        # add fuses into the output norm
        delta = torch.zeros_like(x)
        for blk in self.blocks:
            if self.cfg.gradient_checkpointing and self.training:
                x, delta = torch.utils.checkpoint.checkpoint(
                    blk.forward_pair, x, delta, cos, sin, use_reentrant=False)
            else:
                x, delta = blk.forward_pair(x, delta, cos, sin)
        _, x = ops.add_rmsnorm(x, delta, self.norm.weight, self.norm.eps)
        if self.lm_head is not None:
            logits = self.lm_head(x)
        else:
            logits = torch.nn.functional.linear(x, self.embed.weight)
        if labels is None:
            return logits
        # next-token prediction: shift
        loss = ops.cross_entropy_loss(logits[:, :-1], labels[:, 1:])
        return loss


class RaggedStep:
    """Per-sequence state of one ragged decode step, shared by every layer.

    n_cache int64 [B]: rows sequence b has in the cache = the position of its
    current token; alive bool [B]. A live sequence rotates at n_cache[b],
    appends at row n_cache[b] and attends over n_cache[b] + 1 rows. A finished
    one parks its append out of range (nothing written) and attends over 0
    rows (exact zeros, no cache read). All device tensors: building one costs
    no host round trip, so a step can be graph-captured. t_alloc is the
    parking position: one no append writes at (a contiguous cache's T_max, a
    paged one's max_pages * 64)."""

    __slots__ = ("rope_pos", "append_pos", "attn_lens", "max_len")

    def __init__(self, n_cache: torch.Tensor, alive: torch.Tensor, t_alloc: int,
                 rope_rows: int, max_len: int | None = None):
        self.rope_pos = n_cache.clamp(max=rope_rows - 1)
        self.append_pos = torch.where(alive, n_cache, torch.full_like(n_cache, t_alloc))
        self.attn_lens = torch.where(alive, n_cache + 1,
                                     torch.zeros_like(n_cache)).to(torch.int32)
        self.max_len = max_len

    def attend(self, q, k, v, cos, sin, cache):
        q, k = ops.apply_rope_qk_at(q, k, cos, sin, self.rope_pos)
        cache.append_rows(k, v, self.append_pos)
        if hasattr(cache, "table"):  # paged cache
            return ops.attn_decode_paged(q[:, 0].contiguous(), cache.k, cache.v,
                                         cache.table.table, self.attn_lens,
                                         cache.k_scale, cache.v_scale,
                                         max_len=self.max_len)
        return ops.attn_decode_varlen(q[:, 0].contiguous(), cache.k, cache.v,
                                      self.attn_lens, cache.k_scale, cache.v_scale,
                                      max_len=self.max_len)


def check_prompt_lens(prompt_lens, batch: int, s: int, device) -> torch.Tensor:
    """prompt_lens (list or tensor, int [B], 1 <= L_b <= s) -> int64 [B] on device."""
    lens = torch.as_tensor(prompt_lens).reshape(-1).to(torch.long).cpu()
    if lens.numel() != batch:
        raise ValueError(f"prompt_lens has {lens.numel()} entries for a batch of {batch}")
    if int(lens.min()) < 1 or int(lens.max()) > s:
        raise ValueError(f"prompt_lens must lie in [1, {s}], got {lens.tolist()}")
    return lens.to(device)


def prefill_ragged(model, caches, input_ids, lens, prefill_chunk):
    """Prefill a right-padded batch (possibly in chunks) and return the hidden
    row of every sequence's LAST prompt token [B, 1, h], taken from whichever
    chunk holds it. lens int64 [B] on the device."""
    b, s = input_ids.shape
    seq_lens = lens.to(torch.int32)
    step = s if prefill_chunk is None else prefill_chunk
    rows = torch.arange(b, device=input_ids.device)
    last = None
    for p0 in range(0, s, step):
        x = model.embed(input_ids[:, p0:p0 + step])
        for blk, cache in zip(model.blocks, caches):
            x = blk(x, model.rope_cos, model.rope_sin, cache=cache, pos=p0,
                    seq_lens=seq_lens)
        idx = lens - 1 - p0
        here = (idx >= 0) & (idx < x.shape[1])
        picked = x[rows, idx.clamp(0, x.shape[1] - 1)]
        last = picked if last is None else torch.where(here[:, None], picked, last)
    return last[:, None]


def _sample(logits, temperature, top_k, gen):
    if temperature <= 0:
        return logits.argmax(-1, keepdim=True)
    logits = logits / temperature
    if top_k > 0:
        kth = logits.topk(top_k, dim=-1).values[..., -1, None]
        logits = logits.masked_fill(logits < kth, float("-inf"))
    probs = torch.softmax(logits.float(), dim=-1)
    return torch.multinomial(probs, 1, generator=gen)


def check_sampler(sampler, temperature, top_p, seed) -> None:
    if sampler not in ("multinomial", "philox"):
        raise ValueError(f"sampler must be 'multinomial' or 'philox', got {sampler!r}")
    if sampler == "multinomial":
        if top_p != 1.0:
            raise ValueError("top_p < 1 needs sampler='philox'")
        return
    if seed is None or not temperature > 0:
        raise ValueError("sampler='philox' needs a seed and temperature > 0")
    if not 0 < top_p <= 1:
        raise ValueError(f"top_p must lie in (0, 1], got {top_p}")


def _sample_philox(logits, temperature, top_k, top_p, seed, i):
    """The i-th new token of every row: u = philox_uniform(seed, i, B)."""
    u = ops.philox_uniform(seed, i, logits.shape[0], device=logits.device)
    return ops.sample_token(logits, u, temperature, top_k, top_p)


def _generate_ragged(self, input_ids, max_new_tokens, temperature, top_k, seed,
                     kv_quant, prefill_chunk, prompt_lens, eos_token_id,
                     pad_token_id, top_p=1.0, sampler="multinomial",
                     kv_layout="contiguous", kv_pages=None, kv_free_order=None):
    """Generation over a right-padded batch and/or with a stop token.
    Returns (tokens [B, s + max_new_tokens], lens [B])."""
    from .kv_cache import KVCache
    from .paged_kv import PagedKVCache, PageTable, pages_for

    self.eval()
    b, s = input_ids.shape
    dev = input_ids.device
    total = s + max_new_tokens
    n_cache = check_prompt_lens([s] * b if prompt_lens is None else prompt_lens,
                                b, s, dev)
    # tokens: each prompt, pads everywhere else
    tokens = torch.full((b, total), pad_token_id, dtype=input_ids.dtype, device=dev)
    in_prompt = torch.arange(s, device=dev)[None, :] < n_cache[:, None]
    tokens[:, :s] = torch.where(in_prompt, input_ids, tokens[:, :s])
    lens_out = n_cache.clone()
    if max_new_tokens <= 0:
        return tokens, lens_out
    park = total  # where a finished sequence's append goes: nowhere
    if kv_layout == "paged":
        # every page of the call is reserved here, before the first step:
        # sequence b gets the pages of its own L_b + max_new_tokens rows
        rows = (n_cache + max_new_tokens).tolist()
        need = sum(pages_for(r) for r in rows)
        table = PageTable(b, pages_for(total), need if kv_pages is None else kv_pages,
                          dev, free_order=kv_free_order)
        table.reserve(rows)
        caches = [PagedKVCache(table, self.cfg.n_kv_heads, self.cfg.head_dim, dev,
                               dtype=self.embed.weight.dtype, quant=kv_quant)
                  for _ in self.blocks]
        park = table.max_rows
    else:
        caches = [KVCache(b, total, self.cfg.n_kv_heads, self.cfg.head_dim, dev,
                          dtype=self.embed.weight.dtype, quant=kv_quant)
                  for _ in self.blocks]
    gen = None
    if seed is not None:
        gen = torch.Generator(device=dev).manual_seed(seed)
    alive = torch.ones(b, dtype=torch.bool, device=dev)
    x = prefill_ragged(self, caches, input_ids, n_cache, prefill_chunk)
    for i in range(max_new_tokens):
        x = self.norm(x)
        if self.lm_head is not None:
            logits = self.lm_head(x)[:, 0]
        else:
            logits = torch.nn.functional.linear(x, self.embed.weight)[:, 0]
        if sampler == "philox":
            nxt = _sample_philox(logits, temperature, top_k, top_p, seed, i)
        else:
            nxt = _sample(logits, temperature, top_k, gen)  # [B, 1]
        # a live sequence's new token goes directly after what it has
        at = n_cache.clamp(max=total - 1)[:, None]
        tokens.scatter_(1, at, torch.where(alive[:, None], nxt, tokens.gather(1, at)))
        lens_out = torch.where(alive, n_cache + 1, lens_out)
        if eos_token_id is not None:
            alive = alive & (nxt[:, 0] != eos_token_id)
            if not bool(alive.any()):
                break
        if i == max_new_tokens - 1:
            break
        step = RaggedStep(n_cache, alive, park, self.rope_cos.shape[0],
                          max_len=min(s + i + 1, total))
        x = self.embed(torch.where(alive[:, None], nxt, torch.full_like(nxt, pad_token_id)))
        for blk, cache in zip(self.blocks, caches):
            x = blk(x, self.rope_cos, self.rope_sin, cache=cache, ragged=step)
        n_cache = n_cache + alive.to(n_cache.dtype)
    return tokens, lens_out


@torch.no_grad()
def _generate(self, input_ids: torch.Tensor, max_new_tokens: int = 32,
              temperature: float = 0.0, top_k: int = 0,
              seed: int | None = None, kv_quant: str | None = None,
              prefill_chunk: int | None = None, prompt_lens=None,
              eos_token_id: int | None = None, pad_token_id: int = 0,
              top_p: float = 1.0, sampler: str = "multinomial",
              kv_layout: str = "contiguous", kv_pages: int | None = None,
              kv_free_order=None):
    """Autoregressive generation with a per-layer KV cache (inference parity:
    the reference serves inference through the same executor surface).
    prefill_chunk feeds the prompt in pieces of at most that many tokens
    (activation memory bounded by the chunk); None prefills in one pass.

    prompt_lens (list or tensor, int [B], 1 <= L_b <= s) makes input_ids a
    RIGHT-PADDED batch: row b holds L_b prompt tokens, then anything. The call
    then returns (tokens [B, s + max_new_tokens], lens [B]): each sequence's
    new tokens directly after its own prompt, pad_token_id everywhere else,
    lens[b] its final valid length. eos_token_id stops a sequence once it
    emits that token (kept; pads after it); without prompt_lens the call then
    still returns only tokens.

    sampler="multinomial" (default) draws with torch.multinomial from a
    torch.Generator. sampler="philox" (needs seed and temperature > 0) draws
    the i-th new token of row b from u = ops.philox_uniform(seed, i, B)[b]
    through ops.sample_token, which also provides nucleus sampling (top_p):
    the output is a function of (model, prompt, seed, parameters) alone, the
    same in the graphed decoder.

    kv_layout="paged" keeps the cache in a pool of 64-row pages
    (models/paged_kv.py) instead of one [B, s + max_new_tokens] slab per
    layer: sequence b is charged ceil((L_b + max_new_tokens) / 64) pages,
    reserved before the first step. kv_pages is the pool size (default:
    exactly what the batch needs; too few raise PagePoolExhausted) and
    kv_free_order the order pages are handed out in (default ascending). The
    call always runs the per-sequence route (full lengths without
    prompt_lens) and returns what the contiguous call would."""
    from .kv_cache import KVCache

    check_sampler(sampler, temperature, top_p, seed)
    if prefill_chunk is not None and prefill_chunk < 1:
        raise ValueError(f"prefill_chunk must be >= 1, got {prefill_chunk}")
    if kv_layout not in ("contiguous", "paged"):
        raise ValueError(f"kv_layout must be 'contiguous' or 'paged', got {kv_layout!r}")
    if kv_layout == "paged" or prompt_lens is not None or eos_token_id is not None:
        tokens, lens = _generate_ragged(
            self, input_ids, max_new_tokens, temperature, top_k, seed, kv_quant,
            prefill_chunk, prompt_lens, eos_token_id, pad_token_id, top_p, sampler,
            kv_layout, kv_pages, kv_free_order)
        return (tokens, lens) if prompt_lens is not None else tokens
    self.eval()
    b, s = input_ids.shape
    max_len = s + max_new_tokens
    dtype = self.embed.weight.dtype
    caches = [KVCache(b, max_len, self.cfg.n_kv_heads, self.cfg.head_dim,
                      input_ids.device, dtype=dtype, quant=kv_quant)
              for _ in self.blocks]
    gen = None
    if seed is not None:
        gen = torch.Generator(device=input_ids.device).manual_seed(seed)
    tokens = input_ids
    x_in = input_ids
    pos = 0

    def run_blocks(ids, pos):
        x = self.embed(ids)
        for blk, cache in zip(self.blocks, caches):
            x = blk(x, self.rope_cos, self.rope_sin, cache=cache, pos=pos)
        return x

    # chunked prefill: all pieces but the last only fill the caches; the
    # last piece goes through the loop below and feeds the sampler
    while (prefill_chunk is not None and max_new_tokens > 0
           and x_in.shape[1] > prefill_chunk):
        run_blocks(x_in[:, :prefill_chunk], pos)
        pos += prefill_chunk
        x_in = x_in[:, prefill_chunk:]
    for i in range(max_new_tokens):
        x = run_blocks(x_in, pos)
        x = self.norm(x[:, -1:])
        if self.lm_head is not None:
            logits = self.lm_head(x)[:, 0]
        else:
            logits = torch.nn.functional.linear(x, self.embed.weight)[:, 0]
        if sampler == "philox":
            nxt = _sample_philox(logits, temperature, top_k, top_p, seed, i)
        else:
            nxt = _sample(logits, temperature, top_k, gen)
        pos += x_in.shape[1]
        tokens = torch.cat([tokens, nxt], dim=1)
        x_in = nxt
    return tokens


LlamaForCausalLM.generate = _generate


def build_model(name: str, **overrides) -> LlamaForCausalLM:
    cfg = PRESETS[name]
    if overrides:
        from dataclasses import replace

        cfg = replace(cfg, **overrides)
    return LlamaForCausalLM(cfg)
