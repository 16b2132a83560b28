"""Pure-PyTorch reference implementations of every hot op.

These are (a) the CPU execution path (no GPU in CI), and (b) the fp32 golden
oracle each HIP kernel's numerics test compares against — the pattern the
reference repo uses for its Rust Nesterov pipeline
(/root/reference/crates/worker/src/executor/parameter_server.rs:448-525,
golden-value test vs torch.optim.SGD(nesterov=True)).
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F


# ---------------------------------------------------------------------------
# Normalization
# ---------------------------------------------------------------------------

def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """RMSNorm: x * rsqrt(mean(x^2) + eps) * weight, computed in fp32."""
    dtype = x.dtype
    x32 = x.float()
    var = x32.pow(2).mean(-1, keepdim=True)
    return (x32 * torch.rsqrt(var + eps)).to(dtype) * weight


# ---------------------------------------------------------------------------
# Rotary position embedding (RoPE) — Llama-3 convention: rotate half pairs
# interleaved as (x[..., :d/2], x[..., d/2:]).
# ---------------------------------------------------------------------------

def rope_cos_sin(
    seq_len: int,
    head_dim: int,
    base: float = 500000.0,
    device=None,
    dtype=torch.float32,
) -> tuple[torch.Tensor, torch.Tensor]:
    """Precomputed cos/sin tables of shape [seq_len, head_dim // 2]."""
    inv_freq = 1.0 / (
        base ** (torch.arange(0, head_dim, 2, device=device, dtype=torch.float32) / head_dim)
    )
    t = torch.arange(seq_len, device=device, dtype=torch.float32)
    freqs = torch.outer(t, inv_freq)  # [S, D/2]
    return freqs.cos().to(dtype), freqs.sin().to(dtype)


def apply_rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """Apply RoPE to x of shape [B, H, S, D]; cos/sin are [S, D/2]."""
    d = x.shape[-1] // 2
    x1, x2 = x[..., :d], x[..., d:]
    c = cos[: x.shape[-2]].view(1, 1, -1, d)
    s = sin[: x.shape[-2]].view(1, 1, -1, d)
    out1 = x1.float() * c - x2.float() * s
    out2 = x2.float() * c + x1.float() * s
    return torch.cat([out1, out2], dim=-1).to(x.dtype)


# ---------------------------------------------------------------------------
# Attention (causal, GQA) — reference is plain SDPA-equivalent math
# ---------------------------------------------------------------------------

def attention(
    q: torch.Tensor,  # [B, Hq, S, D]
    k: torch.Tensor,  # [B, Hkv, S, D]
    v: torch.Tensor,  # [B, Hkv, S, D]
    causal: bool = True,
) -> torch.Tensor:
    b, hq, s, d = q.shape
    hkv = k.shape[1]
    if hkv != hq:
        rep = hq // hkv
        k = k.repeat_interleave(rep, dim=1)
        v = v.repeat_interleave(rep, dim=1)
    scale = 1.0 / math.sqrt(d)
    scores = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale
    if causal:
        mask = torch.triu(
            torch.ones(s, s, dtype=torch.bool, device=q.device), diagonal=1
        )
        scores = scores.masked_fill(mask, float("-inf"))
    p = torch.softmax(scores, dim=-1)
    return torch.matmul(p, v.float()).to(q.dtype)


def attention_cached(
    q: torch.Tensor,  # [B, s, Hq, D]  chunk queries, row i at position pos + i
    k: torch.Tensor,  # [B, t, Hkv, D] valid cache prefix, t = pos + s
    v: torch.Tensor,  # [B, t, Hkv, D]
    pos: int,
) -> torch.Tensor:
    """Prefill attention over a KV-cache prefix (bshd): kv index j is visible
    to q row i iff j <= pos + i. fp32 math; returns [B, s, Hq, D] in q.dtype."""
    s, hq, d = q.shape[1], q.shape[2], q.shape[3]
    t = k.shape[1]
    rep = hq // k.shape[2]
    qh = q.transpose(1, 2)  # [B, Hq, s, D]
    kh = k.transpose(1, 2)
    vh = v.transpose(1, 2)
    if rep != 1:
        kh = kh.repeat_interleave(rep, dim=1)
        vh = vh.repeat_interleave(rep, dim=1)
    scores = (qh.float() @ kh.float().transpose(-1, -2)) / math.sqrt(d)
    mask = torch.arange(t, device=q.device)[None, :] > (
        pos + torch.arange(s, device=q.device)[:, None]
    )
    p = torch.softmax(scores.masked_fill(mask, float("-inf")), dim=-1)
    return (p @ vh.float()).to(q.dtype).transpose(1, 2)


PAGE = 64  # rows per KV page (= the kv tile of decode.hip and attn_tile.h)


def gather_pages(pool: torch.Tensor, block_table: torch.Tensor,
                 n_rows: int | None = None) -> torch.Tensor:
    """Contiguous copy of a paged cache: pool [n_pages, 64, ...] and
    block_table int [B, max_pages] -> [B, n_rows, ...], where logical row j of
    sequence b is row j % 64 of page block_table[b, j // 64]. n_rows defaults
    to max_pages * 64. Page ids are clamped to the pool, as the kernels clamp
    them: the rows of a slot no sequence owns hold whatever that page holds."""
    if pool.dim() < 2 or pool.shape[1] != PAGE or block_table.dim() != 2:
        raise ValueError("gather_pages: pool must be [n_pages, 64, ...] and "
                         "block_table [B, max_pages]")
    b, max_pages = block_table.shape
    if n_rows is None:
        n_rows = max_pages * PAGE
    if not 0 <= n_rows <= max_pages * PAGE:
        raise ValueError(f"gather_pages: n_rows={n_rows} outside "
                         f"[0, {max_pages * PAGE}]")
    idx = block_table.to(torch.long).clamp(0, pool.shape[0] - 1)
    fp8 = pool.dtype == torch.float8_e4m3fn  # no fp8 indexing kernel: bytes
    src = pool.view(torch.uint8) if fp8 else pool
    out = src[idx].reshape(b, max_pages * PAGE, *pool.shape[2:])[:, :n_rows]
    out = out.contiguous()
    return out.view(torch.float8_e4m3fn) if fp8 else out


# ---------------------------------------------------------------------------
# SwiGLU MLP activation
# ---------------------------------------------------------------------------

def swiglu(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """silu(gate) * up in fp32."""
    return (F.silu(gate.float()) * up.float()).to(gate.dtype)


def moe_ffn(x: torch.Tensor, router_logits: torch.Tensor, w_gate: torch.Tensor,
            w_up: torch.Tensor, w_down: torch.Tensor, top_k: int) -> torch.Tensor:
    """Top-k routed SwiGLU expert FFN at inference: x [T, h], router_logits
    [T, E], w_gate/w_up [E, f, h], w_down [E, h, f] -> [T, h]. fp32 softmax,
    top-k with the lower index winning ties, weights renormalised to sum 1."""
    logits = router_logits.float()
    probs = torch.softmax(logits, dim=-1)
    topi = torch.sort(logits, dim=-1, descending=True, stable=True).indices[:, :top_k]
    topw = probs.gather(1, topi)
    topw = topw / topw.sum(-1, keepdim=True)
    out = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
    for e in range(w_gate.shape[0]):
        tok, slot = (topi == e).nonzero(as_tuple=True)
        if tok.numel() == 0:
            continue
        xe = x[tok]
        he = swiglu(xe @ w_gate[e].t(), xe @ w_up[e].t())
        ye = (he @ w_down[e].t()).float() * topw[tok, slot].unsqueeze(1)
        out.index_add_(0, tok, ye)
    return out.to(x.dtype)


def linear_fp8w(x: torch.Tensor, w8: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """Weight-only fp8 linear: x [..., K], w8 e4m3 [N, K], scale fp32 [N] ->
    [..., N] in x's dtype. The codes are exact in bf16 and fp32, so the GEMM
    runs on exact weights; the per-row scale is one fp32 multiply after it."""
    return ((x @ w8.to(x.dtype).t()).float() * scale).to(x.dtype)


# the e2m1 magnitudes by code index; an MXFP4 code is sign << 3 | index
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def pow2_f32(e: torch.Tensor) -> torch.Tensor:
    """fp32 2^e for integer e in [-126, 127], built in the exponent field."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


@torch.no_grad()
def dequantize_mxfp4(codes: torch.Tensor, scales: torch.Tensor,
                     dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """The values of MXFP4 codes uint8 [..., K / 2] (two e2m1 per byte, element
    2 i in the low nibble of byte i) and E8M0 scales uint8 [..., K / 32], as
    ops.quantize_mxfp4 produces them -> [..., K] in dtype:
    e2m1(code) * 2^(scale - 127), exactly (every value is a bf16 value)."""
    if (codes.dtype != torch.uint8 or scales.dtype != torch.uint8 or codes.dim() < 1
            or codes.shape[:-1] != scales.shape[:-1]
            or codes.shape[-1] != 16 * scales.shape[-1]):
        raise ValueError("dequantize_mxfp4: codes must be uint8 [..., K / 2] and scales uint8 "
                         "[..., K / 32]")
    nib = torch.stack((codes & 0xf, codes >> 4), -1).reshape(*scales.shape, 32).to(torch.int32)
    # E2M1_VALUES by arithmetic (no table to copy to the device, so the call can
    # be captured in a graph): index i >= 2 is (2 + (i & 1)) 2^(i >> 1) / 4
    idx = nib & 7
    mag = torch.where(idx < 2, idx * 0.5, ((2 + (idx & 1)) << (idx >> 1)) * 0.25)
    vals = torch.where(nib < 8, mag, -mag) * pow2_f32(scales.to(torch.int32) - 127).unsqueeze(-1)
    return vals.reshape(*codes.shape[:-1], 2 * codes.shape[-1]).to(dtype)


def linear_mxfp4w(x: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """Weight-only MXFP4 linear: x [..., K], codes uint8 [N, K / 2], scales
    uint8 [N, K / 32] -> [..., N] in x's dtype. The dequantised weights are
    exact in bf16 and fp32, so the GEMM runs on exact weights."""
    return x @ dequantize_mxfp4(codes, scales, x.dtype).t()


@torch.no_grad()
def quantize_mxfp8(x: torch.Tensor):
    """OCP MXFP8 of finite x [..., K], K % 32 == 0 -> (codes float8_e4m3fn
    [..., K], scales uint8 [..., K / 32]). Each block of 32 consecutive k shares
    the power-of-two scale 2^e, e = floor(log2(amax)) - 8 clamped to
    [-125, 125] (8 is e4m3's largest exponent; a block of zeros takes -125),
    stored as the E8M0 byte e + 127. The code is x * 2^-e (exact in fp32 for
    bf16 x), clamped to +-448 first, so that no cast decides the saturation,
    then rounded to e4m3, ties to even."""
    if not x.is_floating_point() or x.dim() < 1 or x.shape[-1] % 32 != 0:
        raise ValueError("quantize_mxfp8: x must be floating point [..., K] with K % 32 == 0")
    blocks = x.float().reshape(*x.shape[:-1], x.shape[-1] // 32, 32)
    amax = blocks.abs().amax(-1)
    # frexp: amax = m 2^ex with m in [0.5, 1), so floor(log2(amax)) = ex - 1
    e = (torch.frexp(amax).exponent - 9).clamp(-125, 125)
    e = torch.where(amax > 0, e, torch.full_like(e, -125))
    q = (blocks * pow2_f32(-e).unsqueeze(-1)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q.reshape(x.shape), (e + 127).to(torch.uint8)


@torch.no_grad()
def dequantize_mxfp8(codes: torch.Tensor, scales: torch.Tensor,
                     dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """The values of MXFP8 codes float8_e4m3fn [..., K] and E8M0 scales uint8
    [..., K / 32] as quantize_mxfp8 produces them -> [..., K] in dtype:
    e4m3(code) * 2^(scale - 127), exactly (every value is a bf16 value)."""
    if (codes.dtype != torch.float8_e4m3fn or scales.dtype != torch.uint8 or codes.dim() < 1
            or codes.shape[:-1] != scales.shape[:-1]
            or codes.shape[-1] != 32 * scales.shape[-1]):
        raise ValueError("dequantize_mxfp8: codes must be float8_e4m3fn [..., K] and scales "
                         "uint8 [..., K / 32]")
    vals = codes.float().reshape(*scales.shape, 32) * pow2_f32(
        scales.to(torch.int32) - 127).unsqueeze(-1)
    return vals.reshape(codes.shape).to(dtype)


def linear_mxfp4w_a8(x: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """linear_mxfp4w on activations rounded to MXFP8 first: x goes through
    quantize_mxfp8 and back (exactly, in x's dtype for bf16 and wider), then
    meets the dequantised weights in the library's GEMM."""
    xq = dequantize_mxfp8(*quantize_mxfp8(x), x.dtype)
    return xq @ dequantize_mxfp4(codes, scales, x.dtype).t()


def moe_ffn_fp8w(x: torch.Tensor, router_logits: torch.Tensor, w_gate8: torch.Tensor,
                 s_gate: torch.Tensor, w_up8: torch.Tensor, s_up: torch.Tensor,
                 w_down8: torch.Tensor, s_down: torch.Tensor, top_k: int) -> torch.Tensor:
    """moe_ffn on weight-only fp8 experts (codes [E, f, h], [E, f, h], [E, h, f]
    with one fp32 scale per expert and row): the same routing, each projection
    a linear_fp8w."""
    logits = router_logits.float()
    probs = torch.softmax(logits, dim=-1)
    topi = torch.sort(logits, dim=-1, descending=True, stable=True).indices[:, :top_k]
    topw = probs.gather(1, topi)
    topw = topw / topw.sum(-1, keepdim=True)
    out = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
    for e in range(w_gate8.shape[0]):
        tok, slot = (topi == e).nonzero(as_tuple=True)
        if tok.numel() == 0:
            continue
        xe = x[tok]
        he = swiglu(linear_fp8w(xe, w_gate8[e], s_gate[e]), linear_fp8w(xe, w_up8[e], s_up[e]))
        ye = linear_fp8w(he, w_down8[e], s_down[e]).float() * topw[tok, slot].unsqueeze(1)
        out.index_add_(0, tok, ye)
    return out.to(x.dtype)


def moe_ffn_mxfp4w(x: torch.Tensor, router_logits: torch.Tensor, c_gate: torch.Tensor,
                   e_gate: torch.Tensor, c_up: torch.Tensor, e_up: torch.Tensor,
                   c_down: torch.Tensor, e_down: torch.Tensor, top_k: int) -> torch.Tensor:
    """moe_ffn on weight-only MXFP4 experts (codes uint8 [E, f, h / 2],
    [E, f, h / 2], [E, h, f / 2] with E8M0 scales uint8 [..., K / 32]): the same
    routing, each projection a linear_mxfp4w."""
    logits = router_logits.float()
    probs = torch.softmax(logits, dim=-1)
    topi = torch.sort(logits, dim=-1, descending=True, stable=True).indices[:, :top_k]
    topw = probs.gather(1, topi)
    topw = topw / topw.sum(-1, keepdim=True)
    out = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
    for e in range(c_gate.shape[0]):
        tok, slot = (topi == e).nonzero(as_tuple=True)
        if tok.numel() == 0:
            continue
        xe = x[tok]
        he = swiglu(linear_mxfp4w(xe, c_gate[e], e_gate[e]), linear_mxfp4w(xe, c_up[e], e_up[e]))
        ye = linear_mxfp4w(he, c_down[e], e_down[e]).float() * topw[tok, slot].unsqueeze(1)
        out.index_add_(0, tok, ye)
    return out.to(x.dtype)


def moe_ffn_mxfp4w_a8(x: torch.Tensor, router_logits: torch.Tensor, c_gate: torch.Tensor,
                      e_gate: torch.Tensor, c_up: torch.Tensor, e_up: torch.Tensor,
                      c_down: torch.Tensor, e_down: torch.Tensor, top_k: int) -> torch.Tensor:
    """moe_ffn_mxfp4w with both activations rounded to MXFP8 (quantize_mxfp8,
    blocks of 32 consecutive inputs): x before gate and up, v = silu(g) * u
    before down. The same routing, each projection a linear_mxfp4w_a8."""
    logits = router_logits.float()
    probs = torch.softmax(logits, dim=-1)
    topi = torch.sort(logits, dim=-1, descending=True, stable=True).indices[:, :top_k]
    topw = probs.gather(1, topi)
    topw = topw / topw.sum(-1, keepdim=True)
    out = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
    for e in range(c_gate.shape[0]):
        tok, slot = (topi == e).nonzero(as_tuple=True)
        if tok.numel() == 0:
            continue
        xe = x[tok]
        he = swiglu(linear_mxfp4w_a8(xe, c_gate[e], e_gate[e]),
                    linear_mxfp4w_a8(xe, c_up[e], e_up[e]))
        ye = linear_mxfp4w_a8(he, c_down[e], e_down[e]).float() * topw[tok, slot].unsqueeze(1)
        out.index_add_(0, tok, ye)
    return out.to(x.dtype)


# ---------------------------------------------------------------------------
# Cross-entropy over vocab (fp32 logits path)
# ---------------------------------------------------------------------------

def cross_entropy(logits: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """Mean CE over all positions; logits [N, V], targets [N] (-100 ignored)."""
    return F.cross_entropy(logits.float(), targets, ignore_index=-100)


# ---------------------------------------------------------------------------
# Fused inner AdamW (decoupled weight decay) over flat fp32 state
# — oracle for the HIP kernel (K2 in SURVEY.md §2.10)
# ---------------------------------------------------------------------------

@torch.no_grad()
def adamw_step(
    master: torch.Tensor,  # fp32 flat master weights, updated in place
    param_bf16: torch.Tensor,  # bf16 working copy, updated in place
    grad: torch.Tensor,  # grad (any float dtype), same numel
    exp_avg: torch.Tensor,  # fp32 m, in place
    exp_avg_sq: torch.Tensor,  # fp32 v, in place
    *,
    lr: float,
    beta1: float = 0.9,
    beta2: float = 0.95,
    eps: float = 1e-8,
    weight_decay: float = 0.1,
    step: int,
) -> None:
    g = grad.float()
    exp_avg.mul_(beta1).add_(g, alpha=1.0 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    denom = (exp_avg_sq / bc2).sqrt_().add_(eps)
    master.mul_(1.0 - lr * weight_decay)
    master.addcdiv_(exp_avg, denom, value=-lr / bc1)
    param_bf16.copy_(master)


# ---------------------------------------------------------------------------
# Outer Nesterov (DiLoCo aggregate step) over flat fp32 state
# — oracle for the HIP kernel (K7/K8). Matches the reference parameter
#   server's semantics (parameter_server.rs:386-446): with pseudo-gradient
#   delta = theta_t - theta_0 (the *negative* of a gradient), the update is
#     m      <- mu * m + delta
#     theta  <- theta + lr * (mu * m + delta)
#   which equals torch.optim.SGD(lr, momentum=mu, nesterov=True) applied to
#   gradient g = -delta.
# ---------------------------------------------------------------------------

@torch.no_grad()
def nesterov_outer_step(
    master: torch.Tensor,  # fp32 flat global weights (theta_0), in place
    delta: torch.Tensor,  # averaged pseudo-gradient (theta_t - theta_0)
    momentum: torch.Tensor,  # fp32 outer momentum, in place
    *,
    lr: float,
    mu: float = 0.9,
) -> None:
    d = delta.float()
    momentum.mul_(mu).add_(d)
    master.add_(momentum, alpha=lr * mu).add_(d, alpha=lr)


# ---------------------------------------------------------------------------
# Pseudo-gradient extraction / merge (K4/K5):
#   delta = theta_t - theta_0 ; merge: theta <- theta_prev + delta
# (reference: executors/accelerate/.../utils.py:105-123)
# ---------------------------------------------------------------------------

@torch.no_grad()
def extract_delta(theta_t: torch.Tensor, theta_0: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    torch.sub(theta_t, theta_0, out=out)
    return out


# ---------------------------------------------------------------------------
# Token sampling: counter-based Philox4x32-10 uniforms and one deterministic
# function (logits, u) -> token (temperature, top-k, top-p). The HIP kernel
# (ops/hip/sample.hip) computes the same function.
# ---------------------------------------------------------------------------

_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = 0xFFFFFFFF


def _mulhilo32(a: torch.Tensor, m: int):
    """(hi, lo) 32-bit halves of a * m; a int64 holding 32-bit values. 16-bit
    limbs keep every intermediate below 2**63."""
    a0, a1 = a & 0xFFFF, a >> 16
    m0, m1 = m & 0xFFFF, m >> 16
    mid = a1 * m0 + a0 * m1
    low = a0 * m0 + ((mid & 0xFFFF) << 16)
    return (a1 * m1 + (mid >> 16) + (low >> 32)) & _M32, low & _M32


def philox4x32(counter: torch.Tensor, key: torch.Tensor) -> torch.Tensor:
    """Philox4x32-10. counter int64 [..., 4], key int64 [..., 2] (32-bit
    values) -> int64 [..., 4] of 32-bit outputs."""
    c0, c1, c2, c3 = (counter[..., i] & _M32 for i in range(4))
    k0, k1 = key[..., 0] & _M32, key[..., 1] & _M32
    for r in range(10):
        if r:
            k0 = (k0 + _PHILOX_W0) & _M32
            k1 = (k1 + _PHILOX_W1) & _M32
        hi0, lo0 = _mulhilo32(c0, _PHILOX_M0)
        hi1, lo1 = _mulhilo32(c2, _PHILOX_M1)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return torch.stack([c0, c1, c2, c3], dim=-1)


def _scalar(x):
    return x.item() if isinstance(x, torch.Tensor) else x


def philox_uniform(seed, step, n: int, device=None) -> torch.Tensor:
    """fp32 [n]: row r gets u = (x0 >> 8) * 2**-24 with x0 the first output of
    Philox4x32-10 under key (seed & 0xffffffff, seed >> 32) and counter
    (r, step & 0xffffffff, step >> 32, 0)."""
    seed, step = int(_scalar(seed)), int(_scalar(step))
    counter = torch.zeros(n, 4, dtype=torch.long)
    counter[:, 0] = torch.arange(n)
    counter[:, 1] = step & _M32
    counter[:, 2] = (step >> 32) & _M32
    key = torch.tensor([seed & _M32, (seed >> 32) & _M32], dtype=torch.long)
    x0 = philox4x32(counter, key.expand(n, 2))[:, 0]
    u = (x0 >> 8).to(torch.float32) * (2.0 ** -24)
    return u if device is None else u.to(device)


def check_sampling_params(temperature, top_k, top_p) -> None:
    """ValueError for host-visible parameters outside the contract (device
    tensors are not read back here)."""
    if not isinstance(temperature, torch.Tensor) and not temperature > 0:
        raise ValueError(f"sample_token: temperature must be > 0, got {temperature}")
    if not isinstance(top_k, torch.Tensor) and (int(top_k) != top_k or top_k < 0):
        raise ValueError(f"sample_token: top_k must be an int >= 0, got {top_k}")
    if not isinstance(top_p, torch.Tensor) and not 0 < top_p <= 1:
        raise ValueError(f"sample_token: top_p must lie in (0, 1], got {top_p}")


def sample_token(logits: torch.Tensor, u: torch.Tensor, temperature, top_k=0,
                 top_p=1.0) -> torch.Tensor:
    """One token per row of logits [B, V] from the uniform u [B] in [0, 1).

    Tokens are ranked by logit descending, ties by index ascending (-0.0 ==
    +0.0). Mass m_i = exp((z_i - z_max) / temperature) in fp32 (-inf: 0).
    top_k keeps the first k ranked tokens (0 or >= V: off); top_p then keeps
    the shortest ranked prefix whose mass reaches top_p of the kept mass; the
    result is the first kept token whose inclusive cumulative mass (fp64)
    exceeds u times the kept mass, else the last kept token with mass.
    Returns int64 [B, 1]."""
    check_sampling_params(temperature, top_k, top_p)
    t, k, p = float(_scalar(temperature)), int(_scalar(top_k)), float(_scalar(top_p))
    if not t > 0 or not 0 < p <= 1:
        raise ValueError(f"sample_token: temperature={t}, top_p={p} out of range")
    b, v = logits.shape
    z = logits.detach().float() + 0.0  # -0.0 -> +0.0
    zs, idx = torch.sort(z, dim=-1, descending=True, stable=True)
    m = torch.exp((zs - zs[:, :1]) / t)
    m = torch.nan_to_num(m, nan=0.0).masked_fill(zs == float("-inf"), 0.0)
    rank = torch.arange(v, device=logits.device)[None, :]
    n_keep = torch.full((b, 1), k if 0 < k < v else v, device=logits.device)
    c = (m * (rank < n_keep)).double().cumsum(-1)
    if p < 1:
        n_p = (c < p * c[:, -1:]).sum(-1, keepdim=True) + 1
        n_keep = torch.minimum(n_keep, n_p)
    keep = rank < n_keep
    z_kept = c.gather(1, n_keep - 1)
    thresh = u.detach().to(logits.device).double().reshape(b, 1) * z_kept
    hit = keep & (c > thresh)
    first_hit = torch.where(hit, rank, v).amin(-1, keepdim=True)
    last_mass = torch.where(keep & (m > 0), rank, 0).amax(-1, keepdim=True)
    j = torch.where(first_hit < v, first_hit, last_mass)
    return idx.gather(1, j)


# ---------------------------------------------------------------------------
# Stochastic rounding (ops/hip/lean_opt.hip, fp8_lean.hip): the per-element
# hash and the fp32 -> bf16 dither, in int64 arithmetic masked to 32 bits (the
# style of philox4x32), so a test can compare the kernels' rounding decisions
# bit for bit.
# ---------------------------------------------------------------------------

def rnd_hash(idx: torch.Tensor, seed: int) -> torch.Tensor:
    """The kernels' rnd_hash: idx int64 flat element indices (>= 0), seed taken
    mod 2**32 -> int64 holding the 32-bit hash."""
    idx = idx.to(torch.long)
    x = (idx ^ (idx >> 31)) & _M32
    x = (_mulhilo32(x, 0x9E3779B9)[1] + (int(seed) & _M32)) & _M32
    x = x ^ (x >> 16)
    x = _mulhilo32(x, 0x85EBCA6B)[1]
    return x ^ (x >> 13)


def f2bf_sr(f: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """The kernels' f2bf_sr: add the low 16 bits of r below the bf16 mantissa of
    the fp32 f and truncate (NaN -> 0x7fc0). Returns bf16."""
    bits = f.contiguous().view(torch.int32).to(torch.long) & _M32
    out = ((bits + (r & 0xFFFF)) >> 16) & 0xFFFF
    out = torch.where((bits & 0x7FFFFFFF) > 0x7F800000,
                      torch.full_like(out, 0x7FC0), out)
    return ((out ^ 0x8000) - 0x8000).to(torch.int16).view(torch.bfloat16)


@torch.no_grad()
def nesterov_bf16_step(theta: torch.Tensor, delta: torch.Tensor, mom: torch.Tensor,
                       lr: float, mu: float, seed: int):
    """bf16 outer Nesterov chunk (nesterov_bf16_): m = mu*mom + d and
    t = theta + lr*(mu*m + d) in fp32; the kernel stores bf16(m) round-to-nearest
    and theta = f2bf_sr(t, rnd_hash(i, seed)). Returns (t fp32, m fp32, the
    stochastically rounded theta bf16); inputs are not modified."""
    d = delta.float()
    m = mu * mom.float() + d
    t = theta.float() + lr * (mu * m + d)
    idx = torch.arange(t.numel(), device=t.device).view(t.shape)
    return t, m, f2bf_sr(t, rnd_hash(idx, seed))


# ---------------------------------------------------------------------------
# Block-quantised AdamW (ops/hip/adamw8.hip and the lean variants): m as uint8
# codes around 127, sqrt(v) as uint8 codes, one fp32 absmax scale per block.
# ---------------------------------------------------------------------------

QBLOCK = 2048  # elements per quantisation block


def _per_elem(scale: torch.Tensor, n: int) -> torch.Tensor:
    return scale.repeat_interleave(QBLOCK)[:n]


def block_absmax(x: torch.Tensor) -> torch.Tensor:
    """max |x| over each QBLOCK of the flat x (the last block may be partial)."""
    n = x.numel()
    nb = (n + QBLOCK - 1) // QBLOCK
    pad = torch.zeros(nb * QBLOCK, dtype=x.dtype, device=x.device)
    pad[:n] = x.abs()
    return pad.view(nb, QBLOCK).amax(dim=1)


@torch.no_grad()
def adamw8_step(master: torch.Tensor, grad: torch.Tensor, m8: torch.Tensor,
                v8: torch.Tensor, m_scale: torch.Tensor, v_scale: torch.Tensor, *,
                lr: float, beta1: float = 0.9, beta2: float = 0.95,
                eps: float = 1e-8, weight_decay: float = 0.1, step: int):
    """One step of the block-quantised AdamW kernels, in their order of fp32
    operations: dequantise m = (m8 - 127) * ms and v = (v8 * vs)**2, update,
    take each block's absmax, set the new scales am/127 and av/255 (1e-12 when
    the block is all zero) and the new codes with rint and the kernels' clamps.

    master is the fp32 weight going in (the fp32 master, or the dequantised
    bf16/fp8 weight of the lean kernels). Nothing is modified. Returns
    (w, m, sqrt_v, m8_new, v8_new, m_scale_new, v_scale_new); w, m and sqrt_v
    are the fp32 values before any rounding."""
    n = master.numel()
    f32 = dict(dtype=torch.float32, device=master.device)
    one = torch.tensor(1.0, **f32)
    b1, b2 = torch.tensor(beta1, **f32), torch.tensor(beta2, **f32)
    lr32, wd32 = torch.tensor(lr, **f32), torch.tensor(weight_decay, **f32)
    inv_bc1 = one / (one - b1.pow(step))
    inv_bc2 = one / (one - b2.pow(step))
    g = grad.float()
    m = (m8.float() - 127.0) * _per_elem(m_scale, n)
    sv = v8.float() * _per_elem(v_scale, n)
    v = sv * sv
    m = b1 * m + (one - b1) * g
    v = b2 * v + (one - b2) * g * g
    denom = (v * inv_bc2).sqrt() + torch.tensor(eps, **f32)
    w = master.float() * (one - lr32 * wd32) - lr32 * inv_bc1 * m / denom
    sqrt_v = v.sqrt()
    am, av = block_absmax(m), block_absmax(sqrt_v)
    ms_new = torch.where(am > 0, am / 127.0, torch.full_like(am, 1e-12))
    vs_new = torch.where(av > 0, av / 255.0, torch.full_like(av, 1e-12))
    qm = (torch.round(m / _per_elem(ms_new, n)) + 127.0).clamp(0, 254)
    qv = torch.round(sqrt_v / _per_elem(vs_new, n)).clamp(0, 255)
    return w, m, sqrt_v, qm.to(torch.uint8), qv.to(torch.uint8), ms_new, vs_new
