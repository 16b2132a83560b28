"""Public op API: autograd wrappers that dispatch HIP kernels (GPU) or the
PyTorch reference path (CPU).

The HIP extension ABI (hypha_amd._C):
  rmsnorm_fwd(x2d, w, eps) -> (y, rstd)
  rmsnorm_bwd(dy, x2d, w, rstd) -> (dx, dw)
  rope_fwd_ex(q, k, cos, sin, inverse, layout) -> (q_out, k_out)
  swiglu_fwd(gate, up) -> out ; swiglu_bwd(dout, gate, up) -> (dgate, dup)
  ce_fwd(logits2d, targets) -> (loss_sum, lse, n_valid)    # fp32 scalars/rows
  ce_bwd_(logits2d, targets, lse, scale) -> dlogits        # overwrites logits
  attn_fwd_ex(q, k, v, causal, layout) -> (o, lse)         # layout bhsd|bshd
  attn_bwd_ex(q, k, v, o, do, lse, causal, layout) -> (dq, dk, dv)
  attn_decode(q, kcache, vcache, t) -> o                   # + _fp8 / _graph
  attn_prefill(q, kcache, vcache, pos) -> o                # q bshd, any s >= 1
  attn_prefill_fp8(q, kcache, vcache, kscale, vscale, pos) -> o
  attn_decode_varlen(q, kcache, vcache, lens_i32, max_len) -> o   # + _fp8
  attn_prefill_varlen(q, kcache, vcache, pos, seq_lens_i32) -> o  # + _fp8
  kv_append_fp8_(k, v, k8, v8, kscale, vscale, pos_i64[1])
  kv_append_rows_(k, v, kcache, vcache, kscale?, vscale?, pos_i64[B])
  attn_decode_paged(q, kpool, vpool, kscale?, vscale?, table_i32, lens_i32, max_len) -> o
  attn_prefill_paged(q, kpool, vpool, kscale?, vscale?, table_i32, pos, seq_lens_i32?) -> o
  kv_append_paged_(k, v, kpool, vpool, kscale?, vscale?, table_i32, pos_i64, lens_i32?)
  adamw_step_(master, param, grad, m, v, lr, b1, b2, eps, wd, step)
  adamw8_step_(master, param, grad, m8, v8, m_scale, v_scale, ...)  # 8-bit state
  nesterov_step_(master, delta_bf16, momentum, lr, mu)
  extract_delta(master, theta0, out_bf16)
  grad_norm_sq(flat_bf16) -> fp32 scalar
  sample_token(logits_bf16, u_f32, temp_f32[1], top_k_i32[1], top_p_f32[1]) -> int64 [B, 1]
  philox_uniform(seed_i64[1], step_i64[1], n) -> fp32 [n]
"""

from __future__ import annotations

import torch

from . import reference
from . import use_native


def _c():
    from hypha_amd import _C

    return _C


# ---------------------------------------------------------------------------
# RMSNorm
# ---------------------------------------------------------------------------


class _RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        shape = x.shape
        x2d = x.reshape(-1, shape[-1]).contiguous()
        y, rstd = _c().rmsnorm_fwd(x2d, weight, eps)
        ctx.save_for_backward(x2d, weight, rstd)
        ctx.shape = shape
        return y.view(shape)

    @staticmethod
    def backward(ctx, dy):
        x2d, weight, rstd = ctx.saved_tensors
        dx, dw = _c().rmsnorm_bwd(dy.reshape(x2d.shape).contiguous(), x2d, weight, rstd)
        return dx.view(ctx.shape), dw.to(weight.dtype), None


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    if use_native(x):
        return _RMSNorm.apply(x, weight, eps)
    return reference.rmsnorm(x, weight, eps)


class _AddRMSNorm(torch.autograd.Function):
    """Fused h = a + b; y = rmsnorm(h): the residual add is computed inside
    the norm kernel (one fewer elementwise pass per transformer sub-block);
    backward fuses the residual gradient into the dx pass."""

    @staticmethod
    def forward(ctx, a2d, b2d, weight, eps):
        h, y, rstd = _c().add_rmsnorm_fwd(a2d, b2d, weight, eps)
        ctx.save_for_backward(h, weight, rstd)
        return h, y

    @staticmethod
    def backward(ctx, dh, dy):
        h, weight, rstd = ctx.saved_tensors
        if dh is None:
            dx, dw = _c().rmsnorm_bwd(dy.contiguous(), h, weight, rstd)
        else:
            dx, dw = _c().add_rmsnorm_bwd(dy.contiguous(), dh.contiguous(), h,
                                          weight, rstd)
        return dx, dx, dw.to(weight.dtype), None


def add_rmsnorm(a: torch.Tensor, b: torch.Tensor, weight: torch.Tensor,
                eps: float = 1e-5):
    """Returns (h, y) with h = a + b and y = rmsnorm(h), fused on GPU."""
    if use_native(a):
        shape = a.shape
        h, y = _AddRMSNorm.apply(a.reshape(-1, shape[-1]).contiguous(),
                                 b.reshape(-1, shape[-1]).contiguous(),
                                 weight, eps)
        return h.view(shape), y.view(shape)
    h = a + b
    return h, reference.rmsnorm(h, weight, eps)


# ---------------------------------------------------------------------------
# RoPE on q and k together (one fused kernel launch)
# ---------------------------------------------------------------------------


class _RoPE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, cos, sin, layout):
        qo, ko = _c().rope_fwd_ex(q.contiguous(), k.contiguous(), cos, sin, False, layout)
        ctx.save_for_backward(cos, sin)
        ctx.layout = layout
        return qo, ko

    @staticmethod
    def backward(ctx, dq, dk):
        cos, sin = ctx.saved_tensors
        dqo, dko = _c().rope_fwd_ex(dq.contiguous(), dk.contiguous(), cos, sin, True,
                                    ctx.layout)
        return dqo, dko, None, None, None


def apply_rope_qk(q, k, cos, sin, layout: str = "bhsd"):
    """layout 'bhsd': q [B,Hq,S,D]; 'bshd': q [B,S,Hq,D] (the projection's
    natural layout — avoids transpose copies). cos/sin [S_max, D/2] fp32."""
    if use_native(q):
        return _RoPE.apply(q, k, cos, sin, layout)
    if layout == "bshd":
        qo = reference.apply_rope(q.transpose(1, 2), cos, sin).transpose(1, 2)
        ko = reference.apply_rope(k.transpose(1, 2), cos, sin).transpose(1, 2)
        return qo, ko
    return reference.apply_rope(q, cos, sin), reference.apply_rope(k, cos, sin)


def apply_rope_qk_at(q, k, cos, sin, positions):
    """Single-token RoPE at one position per sequence (ragged decode).

    q [B, 1, Hq, D], k [B, 1, Hkv, D] (bshd); positions int64 [B] on q's
    device; cos/sin [S_max, D/2] fp32. Row b is rotated with table row
    positions[b]. The batch is viewed as ONE sequence of B tokens against the
    gathered tables, so the existing kernel (position = token index) serves
    unchanged. Inference only (no autograd)."""
    if q.shape[1] != 1 or k.shape[1] != 1 or positions.shape != (q.shape[0],):
        raise ValueError("apply_rope_qk_at: q/k must be [B, 1, H, D] and "
                         "positions [B]")
    cos_b = cos.index_select(0, positions)  # [B, D/2]
    sin_b = sin.index_select(0, positions)
    q1 = q.reshape(1, *q.shape[:1], *q.shape[2:])  # [1, B, Hq, D]
    k1 = k.reshape(1, *k.shape[:1], *k.shape[2:])
    if use_native(q):
        qo, ko = _c().rope_fwd_ex(q1.contiguous(), k1.contiguous(), cos_b, sin_b,
                                  False, "bshd")
    else:
        qo = reference.apply_rope(q1.transpose(1, 2), cos_b, sin_b).transpose(1, 2)
        ko = reference.apply_rope(k1.transpose(1, 2), cos_b, sin_b).transpose(1, 2)
    return qo.reshape(q.shape), ko.reshape(k.shape)


# ---------------------------------------------------------------------------
# LayerNorm + tanh-GELU (the GPT-2 block's norm/activation)
# ---------------------------------------------------------------------------


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        shape = x.shape
        x2d = x.reshape(-1, shape[-1]).contiguous()
        y, mean, rstd = _c().layernorm_fwd(x2d, weight, bias, eps)
        ctx.save_for_backward(x2d, weight, mean, rstd)
        ctx.shape = shape
        return y.view(shape)

    @staticmethod
    def backward(ctx, dy):
        x2d, weight, mean, rstd = ctx.saved_tensors
        dx, dw, db = _c().layernorm_bwd(dy.reshape(x2d.shape).contiguous(), x2d,
                                        weight, mean, rstd)
        return dx.view(ctx.shape), dw.to(weight.dtype), db.to(weight.dtype), None


def layernorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
              eps: float = 1e-5) -> torch.Tensor:
    if use_native(x):
        return _LayerNorm.apply(x, weight, bias, eps)
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), weight, bias, eps)


class _Gelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        ctx.save_for_backward(x)
        return _c().gelu_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return _c().gelu_bwd(dy.contiguous(), x)


def gelu(x: torch.Tensor) -> torch.Tensor:
    """tanh-approximation GELU (GPT-2's activation)."""
    if use_native(x):
        return _Gelu.apply(x)
    return torch.nn.functional.gelu(x, approximate="tanh")


# ---------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------


class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate, up):
        gate = gate.contiguous()
        up = up.contiguous()
        ctx.save_for_backward(gate, up)
        return _c().swiglu_fwd(gate, up)

    @staticmethod
    def backward(ctx, dout):
        gate, up = ctx.saved_tensors
        dgate, dup = _c().swiglu_bwd(dout.contiguous(), gate, up)
        return dgate, dup


def swiglu(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    if use_native(gate):
        return _SwiGLU.apply(gate, up)
    return reference.swiglu(gate, up)


# ---------------------------------------------------------------------------
# Flash attention (causal, GQA)
# ---------------------------------------------------------------------------


class _FlashAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal, layout):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        o, lse = _c().attn_fwd_ex(q, k, v, causal, layout)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.causal = causal
        ctx.layout = layout
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        dq, dk, dv = _c().attn_bwd_ex(q, k, v, o, do.contiguous(), lse, ctx.causal,
                                      ctx.layout)
        return dq, dk, dv, None, None


def flash_attention(q, k, v, causal: bool = True, layout: str = "bhsd") -> torch.Tensor:
    """Causal GQA attention. layout 'bhsd': q [B,Hq,S,D]; 'bshd': q [B,S,Hq,D]
    (no transpose copies around the projections)."""
    if use_native(q):
        return _FlashAttention.apply(q, k, v, causal, layout)
    if layout == "bshd":
        o = reference.attention(
            q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), causal
        )
        return o.transpose(1, 2)
    return reference.attention(q, k, v, causal)


# ---------------------------------------------------------------------------
# KV-cache decode attention (flash-decoding; serving path)
# ---------------------------------------------------------------------------


def attn_decode(q, kcache, vcache, t: int, kscale=None, vscale=None) -> torch.Tensor:
    """Single-token attention over an appended KV cache.

    q [B, Hq, D] bf16; kcache/vcache [B, T_alloc, Hkv, D] bf16 OR fp8-e4m3
    with per-row scales (bshd); t = valid length including the current
    token. Returns [B, Hq, D] bf16. Native split-KV kernel
    (ops/hip/decode.hip); fp32 reference otherwise.
    """
    quant = kcache.dtype == torch.float8_e4m3fn
    if use_native(q) and q.shape[-1] in (64, 128) and q.shape[1] <= 8 * kcache.shape[2]:
        if quant:
            return _c().attn_decode_fp8(q, kcache, vcache, kscale, vscale, t)
        return _c().attn_decode(q, kcache, vcache, t)
    # reference path (CPU, or head dims the kernel doesn't cover):
    # plain masked softmax over the valid prefix
    if quant:
        kc = kcache[:, :t].float() * kscale[:, :t].unsqueeze(-1).float()
        vc = vcache[:, :t].float() * vscale[:, :t].unsqueeze(-1).float()
    else:
        kc = kcache[:, :t].float()
        vc = vcache[:, :t].float()
    rep = q.shape[1] // kcache.shape[2]
    kh = kc.permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)
    vh = vc.permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)
    scores = torch.einsum("bhd,bhtd->bht", q.float(), kh) / (q.shape[-1] ** 0.5)
    p = torch.softmax(scores, dim=-1)
    o = torch.einsum("bht,bhtd->bhd", p, vh)
    return o.to(q.dtype)


def attn_decode_varlen(q, kcache, vcache, lens, kscale=None, vscale=None,
                       max_len: int | None = None) -> torch.Tensor:
    """Single-token attention with one cache length per sequence.

    q [B, Hq, D] bf16; caches as in attn_decode; lens int32 [B] on q's device,
    lens[b] = valid rows of sequence b INCLUDING the current token (clamped to
    [0, T_alloc]). The kernel reads the lengths at kernel time, so the call is
    graph-capturable as is. lens[b] == 0 returns exact zeros for sequence b
    and reads none of its cache (a finished sequence). max_len (host int,
    default T_alloc) is an upper bound of lens that only sizes the split
    grid. Returns [B, Hq, D] in q's dtype.
    """
    if lens.dtype != torch.int32 or lens.shape != (q.shape[0],):
        raise ValueError("attn_decode_varlen: lens must be int32 [B]")
    t_alloc = kcache.shape[1]
    if max_len is None:
        max_len = t_alloc
    if not 1 <= max_len <= t_alloc:
        raise ValueError(f"attn_decode_varlen: max_len={max_len} outside "
                         f"[1, {t_alloc}]")
    quant = kcache.dtype == torch.float8_e4m3fn
    if quant and (kscale is None or vscale is None):
        raise ValueError("attn_decode_varlen: an fp8 cache needs kscale and vscale")
    if use_native(q) and q.shape[-1] in (64, 128) and q.shape[1] <= 8 * kcache.shape[2]:
        if quant:
            return _c().attn_decode_varlen_fp8(q, kcache, vcache, kscale, vscale,
                                               lens, max_len)
        return _c().attn_decode_varlen(q, kcache, vcache, lens, max_len)
    # reference path: the single-length reference, one sequence at a time
    out = torch.zeros_like(q)
    for b, t in enumerate(lens.clamp(0, t_alloc).tolist()):
        if t == 0:
            continue
        sl = slice(b, b + 1)
        out[sl] = attn_decode(q[sl], kcache[sl], vcache[sl], t,
                              kscale[sl] if quant else None,
                              vscale[sl] if quant else None)
    return out


# ---------------------------------------------------------------------------
# KV-cache prefill attention (ragged prompts, chunked continuation)
# ---------------------------------------------------------------------------


def attn_prefill(q, kcache, vcache, pos: int, kscale=None, vscale=None,
                 seq_lens=None) -> torch.Tensor:
    """Multi-token attention of one prompt chunk over an appended KV cache.

    q [B, s, Hq, D] (bshd), any s >= 1, row i at absolute position pos + i;
    kcache/vcache [B, T_alloc, Hkv, D] bf16 OR fp8-e4m3 with per-row scales
    [B, T_alloc, Hkv], already holding the chunk's own rows, so the valid
    length is t = pos + s and kv j is visible to q row i iff j <= pos + i.
    Returns [B, s, Hq, D] in q's dtype. Native MFMA kernel
    (ops/hip/prefill.hip) on GPU for head dims 64/128; fp32 reference
    otherwise. Inference only (no autograd).

    seq_lens (int32 [B] on q's device; right-padded batches): sequence b is
    valid for len_b = clamp(seq_lens[b], 0, pos + s) rows. kv rows >= len_b
    are masked (and never read by the kernel), q rows at positions >= len_b
    are skipped and their output rows are exact zeros.
    """
    s = q.shape[1]
    t = pos + s
    if pos < 0 or s < 1 or t > kcache.shape[1]:
        raise ValueError(
            f"attn_prefill: pos={pos}, s={s} do not fit a cache of "
            f"{kcache.shape[1]} rows")
    quant = kcache.dtype == torch.float8_e4m3fn
    if quant and (kscale is None or vscale is None):
        raise ValueError("attn_prefill: an fp8 cache needs kscale and vscale")
    if seq_lens is not None and (seq_lens.dtype != torch.int32
                                 or seq_lens.shape != (q.shape[0],)):
        raise ValueError("attn_prefill: seq_lens must be int32 [B]")
    native = (use_native(q) and q.shape[-1] in (64, 128)
              and q.shape[2] % kcache.shape[2] == 0)
    if native and seq_lens is not None:
        if quant:
            return _c().attn_prefill_varlen_fp8(q.contiguous(), kcache, vcache,
                                                kscale, vscale, pos, seq_lens)
        return _c().attn_prefill_varlen(q.contiguous(), kcache, vcache, pos,
                                        seq_lens)
    if native:
        if quant:
            return _c().attn_prefill_fp8(q.contiguous(), kcache, vcache, kscale,
                                         vscale, pos)
        return _c().attn_prefill(q.contiguous(), kcache, vcache, pos)
    # reference path (CPU, or head dims the kernel doesn't cover)
    if quant:
        kc = (kcache[:, :t].float() * kscale[:, :t].unsqueeze(-1)).bfloat16()
        vc = (vcache[:, :t].float() * vscale[:, :t].unsqueeze(-1)).bfloat16()
    else:
        kc, vc = kcache[:, :t], vcache[:, :t]
    if seq_lens is None:
        return reference.attention_cached(q, kc, vc, pos)
    return _attention_cached_varlen(q, kc, vc, pos, seq_lens)


def _attention_cached_varlen(q, k, v, pos: int, seq_lens) -> torch.Tensor:
    """reference.attention_cached with a second mask: kv j is visible to q
    row i of sequence b iff j <= pos + i and j < len_b; rows with
    pos + i >= len_b come out as exact zeros. Masked kv rows are zeroed
    before the matmuls so a non-finite cache tail cannot reach the output."""
    s, d = q.shape[1], q.shape[3]
    t = k.shape[1]
    rep = q.shape[2] // k.shape[2]
    lens = seq_lens.to(torch.long).clamp(0, t)[:, None]  # [B, 1]
    j = torch.arange(t, device=q.device)[None, :]
    i = pos + torch.arange(s, device=q.device)[None, :]
    kv_dead = j >= lens  # [B, t]
    q_dead = i >= lens   # [B, s]
    kh = k.float().masked_fill(kv_dead[:, :, None, None], 0.0).transpose(1, 2)
    vh = v.float().masked_fill(kv_dead[:, :, None, None], 0.0).transpose(1, 2)
    if rep != 1:
        kh = kh.repeat_interleave(rep, dim=1)
        vh = vh.repeat_interleave(rep, dim=1)
    scores = (q.float().transpose(1, 2) @ kh.transpose(-1, -2)) / (d ** 0.5)
    mask = (j[0][None, :] > i[0][:, None])[None] | kv_dead[:, None, :]  # [B, s, t]
    mask = mask & ~q_dead[:, :, None]  # dead rows: keep the softmax finite
    p = torch.softmax(scores.masked_fill(mask[:, None], float("-inf")), dim=-1)
    o = (p @ vh).masked_fill(q_dead[:, None, :, None], 0.0)
    return o.to(q.dtype).transpose(1, 2)


# ---------------------------------------------------------------------------
# Paged KV cache: a pool of 64-row pages and one block table per batch
# ---------------------------------------------------------------------------

PAGE = reference.PAGE


def _check_paged(name, kpool, vpool, block_table, batch, kscale, vscale):
    """Shared argument checks of the paged ops; returns (quant, max_rows)."""
    if (kpool.dim() != 4 or kpool.shape[1] != PAGE or vpool.shape != kpool.shape
            or vpool.dtype != kpool.dtype or kpool.shape[0] < 1):
        raise ValueError(f"{name}: kpool/vpool must be [n_pages, {PAGE}, Hkv, D] "
                         "of one dtype")
    if (block_table.dtype != torch.int32 or block_table.dim() != 2
            or block_table.shape[0] != batch or block_table.shape[1] < 1):
        raise ValueError(f"{name}: block_table must be int32 [B, max_pages]")
    quant = kpool.dtype == torch.float8_e4m3fn
    if quant:
        if kscale is None or vscale is None:
            raise ValueError(f"{name}: an fp8 pool needs kscale and vscale")
        if kscale.shape != kpool.shape[:3] or vscale.shape != kpool.shape[:3]:
            raise ValueError(f"{name}: scales must be [n_pages, {PAGE}, Hkv]")
    return quant, block_table.shape[1] * PAGE


def attn_decode_paged(q, kpool, vpool, block_table, lens, kscale=None, vscale=None,
                      max_len: int | None = None) -> torch.Tensor:
    """attn_decode_varlen over a paged cache.

    q [B, Hq, D] bf16; kpool/vpool [n_pages, 64, Hkv, D] bf16 OR fp8-e4m3 with
    scales [n_pages, 64, Hkv]; block_table int32 [B, max_pages] on q's device:
    logical row j of sequence b is row j % 64 of page block_table[b, j // 64].
    lens int32 [B] as in attn_decode_varlen, clamped to [0, max_pages * 64];
    table slots at or past ceil(lens[b] / 64) are never read, the ones read are
    clamped to the pool, and lens[b] == 0 reads neither table nor pool. max_len
    (default max_pages * 64) only sizes the split grid. Graph-capturable as is.
    For the same logical cache and the same max_len the native kernel's output
    equals attn_decode_varlen's bit for bit (the kernel body is shared;
    ops/hip/decode.hip). Returns [B, Hq, D] in q's dtype.
    """
    if q.dim() != 3:
        raise ValueError("attn_decode_paged: q must be [B, Hq, D]")
    quant, max_rows = _check_paged("attn_decode_paged", kpool, vpool, block_table,
                                   q.shape[0], kscale, vscale)
    if lens.dtype != torch.int32 or lens.shape != (q.shape[0],):
        raise ValueError("attn_decode_paged: lens must be int32 [B]")
    if max_len is None:
        max_len = max_rows
    if not 1 <= max_len <= max_rows:
        raise ValueError(f"attn_decode_paged: max_len={max_len} outside "
                         f"[1, {max_rows}]")
    if use_native(q) and q.shape[-1] in (64, 128) and q.shape[1] <= 8 * kpool.shape[2]:
        return _c().attn_decode_paged(q, kpool, vpool, kscale if quant else None,
                                      vscale if quant else None, block_table, lens,
                                      max_len)
    # reference path: the contiguous reference on the gathered pages
    g = reference.gather_pages
    return attn_decode_varlen(
        q, g(kpool, block_table), g(vpool, block_table), lens,
        g(kscale, block_table) if quant else None,
        g(vscale, block_table) if quant else None, max_len=max_len)


def attn_prefill_paged(q, kpool, vpool, block_table, pos: int, kscale=None,
                       vscale=None, seq_lens=None) -> torch.Tensor:
    """attn_prefill over a paged cache (pools and block_table as in
    attn_decode_paged). q [B, s, Hq, D], row i at absolute position pos + i;
    needs pos + s <= max_pages * 64; the chunk's own rows are already
    appended. seq_lens as in attn_prefill. A tile's page is looked up only
    when the tile holds a row below the sequence's bound, so slots past a
    sequence's pages are never read. For the same logical cache the native
    kernel's output equals attn_prefill's bit for bit (ops/hip/prefill.hip).
    """
    if q.dim() != 4:
        raise ValueError("attn_prefill_paged: q must be [B, s, Hq, D]")
    quant, max_rows = _check_paged("attn_prefill_paged", kpool, vpool, block_table,
                                   q.shape[0], kscale, vscale)
    s = q.shape[1]
    if pos < 0 or s < 1 or pos + s > max_rows:
        raise ValueError(f"attn_prefill_paged: pos={pos}, s={s} do not fit "
                         f"{max_rows} rows of pages")
    if seq_lens is not None and (seq_lens.dtype != torch.int32
                                 or seq_lens.shape != (q.shape[0],)):
        raise ValueError("attn_prefill_paged: seq_lens must be int32 [B]")
    if (use_native(q) and q.shape[-1] in (64, 128)
            and q.shape[2] % kpool.shape[2] == 0):
        return _c().attn_prefill_paged(q.contiguous(), kpool, vpool,
                                       kscale if quant else None,
                                       vscale if quant else None, block_table, pos,
                                       seq_lens)
    g = reference.gather_pages
    return attn_prefill(
        q, g(kpool, block_table), g(vpool, block_table), pos,
        g(kscale, block_table) if quant else None,
        g(vscale, block_table) if quant else None, seq_lens=seq_lens)


def quantize_rows_e4m3(x: torch.Tensor):
    """x [..., D] -> (e4m3 [..., D], fp32 scale [...]): KVCache._quantize_rows'
    arithmetic (scale = amax / 448, elements divided by the scale)."""
    amax = x.float().abs().amax(-1).clamp(min=1e-8)
    scale = amax / 448.0
    q = (x.float() / scale.unsqueeze(-1)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q, scale


def kv_append_paged(k, v, kpool, vpool, block_table, pos, kscale=None, vscale=None,
                    lens=None) -> None:
    """Append k/v [B, s, Hkv, D] (s >= 1) into a paged cache, in place.

    Row i of sequence b goes to logical position p = pos[b] + i (pos: int64
    [B] on k's device, or int64 [1] / a Python int for one position for the
    whole batch), i.e. row p % 64 of page block_table[b, p // 64]. The row is
    written iff 0 <= p < max_pages * 64, the page id lies in [0, n_pages), and
    p < lens[b] when lens (int32 [B]) is given: a right-padded chunk then
    writes no pad rows, and a parked sequence (position at or past
    max_pages * 64) writes nothing. An fp8 pool stores the bytes and scales of
    KVCache._quantize_rows, bit for bit. With pos on the device the call is
    graph-capturable (ops/hip/decode.hip kv_append_paged_*_kernel).
    """
    if k.dim() != 4 or v.shape != k.shape or k.shape[1] < 1:
        raise ValueError("kv_append_paged: k/v must be [B, s, Hkv, D], s >= 1")
    b, s = k.shape[:2]
    quant, max_rows = _check_paged("kv_append_paged", kpool, vpool, block_table, b,
                                   kscale, vscale)
    if kpool.shape[2:] != k.shape[2:]:
        raise ValueError("kv_append_paged: k/v and the pools differ in [Hkv, D]")
    if not isinstance(pos, torch.Tensor):
        pos = torch.tensor([int(pos)], dtype=torch.long, device=k.device)
    if pos.dtype != torch.long or pos.dim() != 1 or pos.shape[0] not in (1, b):
        raise ValueError("kv_append_paged: pos must be int64 [1] or [B]")
    if lens is not None and (lens.dtype != torch.int32 or lens.shape != (b,)):
        raise ValueError("kv_append_paged: lens must be int32 [B]")
    d = k.shape[-1]
    if (use_native(k) and k.dtype == torch.bfloat16
            and (d in (64, 128) if quant else
                 (kpool.dtype == torch.bfloat16 and d % 8 == 0))):
        _c().kv_append_paged_(k.contiguous(), v.contiguous(), kpool, vpool,
                              kscale if quant else None, vscale if quant else None,
                              block_table, pos, lens)
        return
    # reference path: the same row selection in PyTorch
    n_pages = kpool.shape[0]
    p = pos.expand(b)[:, None] + torch.arange(s, device=k.device)[None, :]  # [B, s]
    ok = (p >= 0) & (p < max_rows)
    if lens is not None:
        ok &= p < lens.to(torch.long)[:, None]
    page = block_table.to(torch.long).gather(
        1, (p // PAGE).clamp(0, block_table.shape[1] - 1))
    ok &= (page >= 0) & (page < n_pages)
    rows = (page * PAGE + p % PAGE)[ok]  # flat pool rows of the written (b, i)
    for x, pool, scale in ((k, kpool, kscale), (v, vpool, vscale)):
        flat = pool.view(torch.uint8) if quant else pool
        flat = flat.view(n_pages * PAGE, *pool.shape[2:])
        if quant:
            xq, sc = quantize_rows_e4m3(x[ok])
            flat[rows] = xq.view(torch.uint8)
            scale.view(n_pages * PAGE, -1)[rows] = sc
        else:
            flat[rows] = x[ok].to(pool.dtype)


def linear_skinny(x2d: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """Inference linear for decode shapes: out = x2d @ weight.T with the
    weight-bandwidth-bound skinny-M kernel when M <= 8 (ops/hip/
    skinny_gemm.hip); hipBLASLt otherwise. No autograd."""
    if (use_native(x2d) and x2d.shape[0] <= 8
            and weight.dtype == torch.bfloat16):
        return _c().skinny_gemm(x2d.contiguous(), weight)
    return x2d @ weight.t()


# ---------------------------------------------------------------------------
# Token sampling (temperature / top-k / top-p) and its Philox uniforms
# ---------------------------------------------------------------------------


def _dev_scalar(x, dtype, device) -> torch.Tensor:
    """A Python number or a 1-element tensor -> 1-element tensor on device
    (no host round trip for a tensor already there)."""
    if isinstance(x, torch.Tensor):
        return x.reshape(1).to(device=device, dtype=dtype)
    return torch.tensor([x], dtype=dtype, device=device)


@torch.no_grad()
def sample_token(logits: torch.Tensor, u: torch.Tensor, temperature, top_k=0,
                 top_p=1.0) -> torch.Tensor:
    """One token per row: logits [B, V], u fp32 [B] in [0, 1) -> int64 [B, 1].

    A pure function of (logits, u), the same on CPU and GPU (contract:
    reference.sample_token): rank by logit descending, ties by index
    ascending; top_k keeps the first k (0 or >= V: off); top_p in (0, 1] then
    keeps the shortest prefix reaching that share of the kept mass; u picks by
    inverse CDF. temperature > 0 (greedy is the caller's argmax). The three
    parameters may be Python numbers (validated: ValueError) or 1-element
    device tensors (read by the kernel at kernel time, so a captured graph
    serves every setting). Native kernel (ops/hip/sample.hip) for contiguous
    bf16 GPU logits; the reference for everything else."""
    reference.check_sampling_params(temperature, top_k, top_p)
    if not isinstance(top_k, torch.Tensor):
        top_k = min(int(top_k), 2 ** 31 - 1)
    if logits.dim() != 2 or u.numel() != logits.shape[0]:
        raise ValueError("sample_token: logits must be [B, V] and u [B]")
    if (logits.dtype == torch.bfloat16 and logits.is_contiguous()
            and use_native(logits)):
        dev = logits.device
        return _c().sample_token(
            logits, u.reshape(-1).to(device=dev, dtype=torch.float32).contiguous(),
            _dev_scalar(temperature, torch.float32, dev),
            _dev_scalar(top_k, torch.int32, dev),
            _dev_scalar(top_p, torch.float32, dev))
    return reference.sample_token(logits, u, temperature, top_k, top_p)


@torch.no_grad()
def philox_uniform(seed, step, n: int, device=None) -> torch.Tensor:
    """fp32 [n] uniforms in [0, 1): row r of Philox4x32-10 with key
    (seed & 0xffffffff, seed >> 32) and counter (r, step & 0xffffffff,
    step >> 32, 0), u = (x0 >> 8) * 2**-24. seed and step are ints or
    1-element int64 tensors; device defaults to theirs (else the CPU)."""
    if device is None:
        device = next((x.device for x in (seed, step)
                       if isinstance(x, torch.Tensor)), torch.device("cpu"))
    device = torch.device(device)
    if device.type == "cuda" and use_native(torch.empty(0, device=device)):
        return _c().philox_uniform(_dev_scalar(seed, torch.long, device),
                                   _dev_scalar(step, torch.long, device), int(n))
    return reference.philox_uniform(seed, step, n, device=device)


# ---------------------------------------------------------------------------
# Cross-entropy over vocab (memory-frugal: backward overwrites the logits)
# ---------------------------------------------------------------------------


class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits2d, targets):
        loss_sum, lse, n_valid = _c().ce_fwd(logits2d, targets)
        ctx.save_for_backward(logits2d, targets, lse)
        ctx.n_valid = max(int(n_valid), 1)
        return loss_sum / ctx.n_valid

    @staticmethod
    def backward(ctx, dloss):
        logits2d, targets, lse = ctx.saved_tensors
        scale = float(dloss) / ctx.n_valid
        dlogits = _c().ce_bwd_(logits2d, targets, lse, scale)
        return dlogits, None


def cross_entropy_loss(logits: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """logits [..., V], targets [...] int64 with -100 = ignore. Mean loss."""
    v = logits.shape[-1]
    logits2d = logits.reshape(-1, v)
    t = targets.reshape(-1)
    if use_native(logits):
        return _CrossEntropy.apply(logits2d.contiguous(), t.contiguous())
    return reference.cross_entropy(logits2d, t)


# ---------------------------------------------------------------------------
# Fused optimizers (no autograd; flat-buffer in-place)
# ---------------------------------------------------------------------------


@torch.no_grad()
def fused_adamw(master, param, grad, exp_avg, exp_avg_sq, *, lr, beta1, beta2, eps, weight_decay, step):
    if use_native(master):
        _c().adamw_step_(master, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step)
    else:
        reference.adamw_step(
            master, param, grad, exp_avg, exp_avg_sq,
            lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay, step=step,
        )


@torch.no_grad()
def fused_nesterov(master, delta, momentum, *, lr, mu):
    if use_native(master):
        _c().nesterov_step_(master, delta, momentum, lr, mu)
    else:
        reference.nesterov_outer_step(master, delta, momentum, lr=lr, mu=mu)


@torch.no_grad()
def extract_delta(master: torch.Tensor, theta0: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out (bf16 or fp32) = master - theta0, fused sub+cast on GPU."""
    if use_native(master):
        _c().extract_delta(master, theta0, out)
        return out
    out.copy_(master - theta0)
    return out
