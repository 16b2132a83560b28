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
