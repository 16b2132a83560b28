"""Textbook fp64 forwards of the three model families, for the parity tests.

Plain functions of (parameters as fp64, config, ids, labels) -> (logits, loss)
written from the architectures' definitions with ordinary torch ops: plain
residual adds, no (residual, delta) carry, no fused kernels, no KV cache.
Nothing here imports hypha_amd.models or hypha_amd.ops, so an error in the
models' wiring or in an op cannot cancel against the same error here.

P is params64(model): every named parameter and the RoPE tables (the model's
own fp32 tables cast to fp64, so table rounding is on neither side of a
comparison), fp64 on the CPU. A config is read by attribute only.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F


# ---- parameters and initialisation -----------------------------------------


@torch.no_grad()
def unit_gain_(model, seed: int):
    """Re-initialise so that every sub-block passes its input on at unit gain:
    attention and the MLPs then reach the logits at full strength, where the
    default init (std 0.02) buries them below bf16 rounding.

    2-D (and per-expert 3-D) weights ~ N(0, 1/fan_in); embeddings ~ N(0, 1);
    norm weights 1 + 0.1 N(0, 1); biases 0.1 N(0, 1); all rounded to bf16
    values, so a bf16 copy of the model holds exactly these numbers."""
    g = torch.Generator().manual_seed(seed)
    emb = {id(m.weight) for m in model.modules() if isinstance(m, torch.nn.Embedding)}
    for name, p in model.named_parameters():
        z = torch.randn(p.shape, generator=g)
        if id(p) in emb:
            val = z
        elif p.dim() >= 2:
            val = z / math.sqrt(p.shape[-1])
        elif name.endswith("bias"):
            val = 0.1 * z
        else:
            val = 1.0 + 0.1 * z
        p.copy_(val.bfloat16().to(p.dtype))
    return model


def params64(model, requires_grad: bool = False) -> dict:
    """Named parameters and RoPE tables as fp64 CPU leaves."""
    P = {n: p.detach().cpu().double().requires_grad_(requires_grad)
         for n, p in model.named_parameters()}
    for n, b in model.named_buffers():
        if n in ("rope_cos", "rope_sin"):
            P[n] = b.detach().cpu().double()
    return P


def make_batch(vocab: int, b: int, s: int, seed: int):
    """ids [b, s] and labels = ids with about one sixth of the positions -100."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, vocab, (b, s), generator=g)
    labels = ids.clone()
    labels[torch.rand(b, s, generator=g) < 1.0 / 6.0] = -100
    return ids, labels


# ---- metrics ---------------------------------------------------------------


def rel_l2(a, b) -> float:
    """|a - b| / |b| over the whole tensor, in fp64; b is the reference."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    den = b.norm().item()
    num = (a - b).norm().item()
    if den == 0.0:
        return 0.0 if num == 0.0 else float("inf")
    return num / den


def worst_row(a, b) -> float:
    """Maximum over the rows of the last dimension of the row-wise rel-L2."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).norm(dim=-1) / b.norm(dim=-1)).max().item()


def grad_rel_l2(grads: dict, ref: dict) -> dict:
    """Per-parameter rel-L2 of grads[name] against ref[name]."""
    return {n: rel_l2(grads[n], ref[n]) for n in ref}


# ---- shared pieces ---------------------------------------------------------


def rms64(x, w, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def rope64(x, cos, sin):
    """Rotate-half RoPE; x [B, S, H, D], row s rotated by table row s."""
    d = x.shape[-1] // 2
    c = cos[: x.shape[1]][None, :, None, :]
    s = sin[: x.shape[1]][None, :, None, :]
    x1, x2 = x[..., :d], x[..., d:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


def causal_attention64(q, k, v):
    """q [B, S, Hq, D], k/v [B, S, Hkv, D]; query head h reads kv head
    h // (Hq / Hkv). Returns [B, S, Hq * D]."""
    b, s, hq, d = q.shape
    rep = hq // k.shape[2]
    qh = q.transpose(1, 2)
    kh = k.transpose(1, 2).repeat_interleave(rep, 1)
    vh = v.transpose(1, 2).repeat_interleave(rep, 1)
    sc = qh @ kh.transpose(-1, -2) / math.sqrt(d)
    sc = sc.masked_fill(torch.ones(s, s, dtype=torch.bool).triu(1), float("-inf"))
    return (torch.softmax(sc, -1) @ vh).transpose(1, 2).reshape(b, s, hq * d)


def shifted_ce64(logits, labels):
    """Mean next-token CE over the positions whose label is not -100."""
    v = logits.shape[-1]
    return F.cross_entropy(logits[:, :-1].reshape(-1, v), labels[:, 1:].reshape(-1),
                           ignore_index=-100)


def _llama_attention(P, pre, cfg, h):
    b, s, _ = h.shape
    hd = cfg.hidden_size // cfg.n_heads
    q = (h @ P[pre + "attn.wq.weight"].T).view(b, s, cfg.n_heads, hd)
    k = (h @ P[pre + "attn.wk.weight"].T).view(b, s, cfg.n_kv_heads, hd)
    v = (h @ P[pre + "attn.wv.weight"].T).view(b, s, cfg.n_kv_heads, hd)
    q = rope64(q, P["rope_cos"], P["rope_sin"])
    k = rope64(k, P["rope_cos"], P["rope_sin"])
    return causal_attention64(q, k, v) @ P[pre + "attn.wo.weight"].T


# ---- Llama -----------------------------------------------------------------


def llama64(P, cfg, ids, labels=None):
    x = P["embed.weight"][ids]
    for i in range(cfg.n_layers):
        pre = f"blocks.{i}."
        x = x + _llama_attention(P, pre, cfg, rms64(x, P[pre + "attn_norm.weight"],
                                                    cfg.norm_eps))
        h = rms64(x, P[pre + "mlp_norm.weight"], cfg.norm_eps)
        g = h @ P[pre + "mlp.w_gate.weight"].T
        u = h @ P[pre + "mlp.w_up.weight"].T
        x = x + (F.silu(g) * u) @ P[pre + "mlp.w_down.weight"].T
    x = rms64(x, P["norm.weight"], cfg.norm_eps)
    head = P["embed.weight"] if cfg.tie_embeddings else P["lm_head.weight"]
    logits = x @ head.T
    return logits, (None if labels is None else shifted_ce64(logits, labels))


# ---- GPT-2 -----------------------------------------------------------------


def gpt2_64(P, cfg, ids, labels=None):
    b, s = ids.shape
    hsz, nh = cfg.hidden_size, cfg.n_heads
    ln = lambda x, n: F.layer_norm(x, (hsz,), P[n + ".weight"], P[n + ".bias"],  # noqa: E731
                                   cfg.norm_eps)
    x = P["wte.weight"][ids] + P["wpe.weight"][:s]
    for i in range(cfg.n_layers):
        pre = f"blocks.{i}."
        qkv = ln(x, pre + "ln1") @ P[pre + "attn_qkv.weight"].T + P[pre + "attn_qkv.bias"]
        q, k, v = (t.view(b, s, nh, hsz // nh) for t in qkv.split(hsz, dim=-1))
        o = causal_attention64(q, k, v)
        x = x + o @ P[pre + "attn_out.weight"].T + P[pre + "attn_out.bias"]
        a = ln(x, pre + "ln2") @ P[pre + "mlp_fc.weight"].T + P[pre + "mlp_fc.bias"]
        a = 0.5 * a * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (a + 0.044715 * a ** 3)))
        x = x + a @ P[pre + "mlp_proj.weight"].T + P[pre + "mlp_proj.bias"]
    logits = ln(x, "ln_f") @ P["wte.weight"].T
    return logits, (None if labels is None else shifted_ce64(logits, labels))


# ---- MoE -------------------------------------------------------------------


def moe64(P, cfg, ids, labels=None, routing=None, training=False):
    """Returns (logits, loss, own): own[l] int64 [T, K] is this function's fp64
    top-k choice in layer l, best first.

    Routing is discrete, so a run in another precision may choose differently
    at a near tie and is then a different function. routing[l] (int64 [T, K],
    best first, T = B * S tokens in row-major order) therefore fixes WHICH
    experts layer l uses; the weights are this function's own fp64 router
    probabilities of those experts, renormalised. routing=None uses own.

    training adds the Switch load-balancing term per layer,
    coef * E * sum_e mean_t(p[t, e]) * mean_t(first choice of t is e),
    to the loss."""
    x = P["embed.weight"][ids]
    b, s, hsz = x.shape
    own, aux = [], x.new_zeros(())
    for i in range(cfg.n_layers):
        pre = f"blocks.{i}."
        x = x + _llama_attention(P, pre, cfg, rms64(x, P[pre + "attn_norm.weight"],
                                                    cfg.norm_eps))
        h = rms64(x, P[pre + "mlp_norm.weight"], cfg.norm_eps).reshape(-1, hsz)
        probs = torch.softmax(h @ P[pre + "mlp.router.weight"].T, -1)  # [T, E]
        own.append(probs.topk(cfg.top_k, -1).indices)
        idx = own[-1] if routing is None else routing[i]
        w = probs.gather(1, idx)
        w = w / w.sum(-1, keepdim=True)
        if training:
            first = F.one_hot(idx[:, 0], cfg.n_experts).double().mean(0)
            aux = aux + cfg.router_aux_loss_coef * cfg.n_experts * (probs.mean(0) * first).sum()
        out = torch.zeros_like(h)
        for e in range(cfg.n_experts):
            tok, slot = (idx == e).nonzero(as_tuple=True)
            he = h[tok]
            ge = he @ P[pre + "mlp.w_gate"][e].T
            ue = he @ P[pre + "mlp.w_up"][e].T
            ye = (F.silu(ge) * ue) @ P[pre + "mlp.w_down"][e].T
            out = out.index_add(0, tok, ye * w[tok, slot][:, None])
        x = x + out.view(b, s, hsz)
    logits = rms64(x, P["norm.weight"], cfg.norm_eps) @ P["lm_head.weight"].T
    loss = None
    if labels is not None:
        loss = shifted_ce64(logits, labels)
        if training:
            loss = loss + aux
    return logits, loss, own


def topk_sets(router_logits, k: int):
    """The model's routing of one layer from its router's output: softmax in
    fp32, then top-k (best first). int64 [T, K] on the CPU."""
    probs = torch.softmax(router_logits.detach().float(), dim=-1)
    return probs.topk(k, dim=-1).indices.cpu()


def routing_agreement(a, b) -> float:
    """Share of tokens whose top-k SETS are equal."""
    return (a.sort(-1).values == b.sort(-1).values).all(-1).double().mean().item()


# ---- the configurations the parity tests share ------------------------------

# name -> (registry name, overrides, sequence length)
CONFIGS = {
    # 4 heads over 2 kv heads, D = 64, untied
    "L1": ("llama-tiny", dict(hidden_size=256, n_heads=4, n_kv_heads=2, ffn_hidden=512,
                              n_layers=2), 128),
    # D = 128, tied head, checkpointing, an odd number of pair carries, two
    # q tiles and one 256-key backward block
    "L2": ("llama-tiny", dict(hidden_size=256, n_heads=2, n_kv_heads=1, n_layers=3,
                              tie_embeddings=True, gradient_checkpointing=True), 256),
    "G1": ("gpt2-tiny", dict(vocab_size=512, n_positions=256, hidden_size=128,
                             n_layers=2, n_heads=2), 128),
    "M1": ("moe-tiny", dict(hidden_size=128, n_heads=2, n_kv_heads=2, n_experts=4,
                            top_k=2, ffn_hidden=256, n_layers=2), 128),
    # generation only: L2's attention shape with an untied head
    "L2u": ("llama-tiny", dict(hidden_size=256, n_heads=2, n_kv_heads=1, n_layers=3), 256),
}
BATCH = 2
# one seed per configuration, for weights (seed) and batch (seed + 1)
SEEDS = {"L1": 0, "L2": 0, "G1": 0, "M1": 0, "L2u": 0}
TEXTBOOK = {"L1": llama64, "L2": llama64, "L2u": llama64, "G1": gpt2_64, "M1": moe64}
