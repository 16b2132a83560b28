"""CPU tests of the reference op implementations and their gradients."""

import math

import pytest
import torch
import torch.nn.functional as F

from hypha_amd.ops import reference as R


def test_rmsnorm_matches_torch():
    x = torch.randn(4, 64)
    w = torch.randn(64)
    got = R.rmsnorm(x, w, eps=1e-5)
    want = F.rms_norm(x, (64,), weight=w, eps=1e-5)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)


def test_rope_rotation_preserves_norm():
    cos, sin = R.rope_cos_sin(32, 16, base=10000.0)
    x = torch.randn(2, 4, 32, 16)
    y = R.apply_rope(x, cos, sin)
    torch.testing.assert_close(
        x.norm(dim=-1), y.norm(dim=-1), rtol=1e-5, atol=1e-5
    )
    # position 0 is identity
    torch.testing.assert_close(y[:, :, 0], x[:, :, 0], rtol=1e-6, atol=1e-6)


def test_rope_inverse():
    cos, sin = R.rope_cos_sin(32, 16, base=10000.0)
    x = torch.randn(1, 2, 32, 16)
    y = R.apply_rope(x, cos, sin)
    back = R.apply_rope(y, cos, -sin)
    torch.testing.assert_close(back, x, rtol=1e-5, atol=1e-5)


def test_attention_matches_sdpa():
    torch.manual_seed(0)
    q = torch.randn(2, 4, 16, 8)
    k = torch.randn(2, 2, 16, 8)
    v = torch.randn(2, 2, 16, 8)
    got = R.attention(q, k, v, causal=True)
    want = F.scaled_dot_product_attention(
        q, k.repeat_interleave(2, 1), v.repeat_interleave(2, 1), is_causal=True
    )
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5)


def test_swiglu():
    g = torch.randn(8, 16)
    u = torch.randn(8, 16)
    torch.testing.assert_close(R.swiglu(g, u), F.silu(g) * u, rtol=1e-5, atol=1e-6)


def test_cross_entropy_ignore_index():
    logits = torch.randn(6, 11)
    t = torch.tensor([1, 2, -100, 4, 5, -100])
    torch.testing.assert_close(
        R.cross_entropy(logits, t), F.cross_entropy(logits, t, ignore_index=-100)
    )


def test_adamw_matches_torch_optim():
    torch.manual_seed(1)
    n = 257
    master = torch.randn(n)
    p_ref = master.clone().requires_grad_(True)
    opt = torch.optim.AdamW(
        [p_ref], lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1
    )
    param = master.clone()
    m = torch.zeros(n)
    v = torch.zeros(n)
    for step in range(1, 6):
        g = torch.randn(n)
        p_ref.grad = g.clone()
        opt.step()
        R.adamw_step(
            master, param, g, m, v,
            lr=1e-2, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.1, step=step,
        )
    torch.testing.assert_close(master, p_ref.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(param, master)


def test_nesterov_matches_torch_sgd():
    """The golden-value pattern from the reference parameter server
    (parameter_server.rs:448-525): our outer step with pseudo-gradient
    delta must equal torch SGD(nesterov=True) fed gradient -delta."""
    torch.manual_seed(2)
    n = 97
    theta = torch.randn(n)
    p_ref = theta.clone().requires_grad_(True)
    opt = torch.optim.SGD([p_ref], lr=0.7, momentum=0.9, nesterov=True)
    momentum = torch.zeros(n)
    for _ in range(4):
        delta = torch.randn(n)
        p_ref.grad = -delta
        opt.step()
        R.nesterov_outer_step(theta, delta, momentum, lr=0.7, mu=0.9)
    torch.testing.assert_close(theta, p_ref.detach(), rtol=1e-5, atol=1e-6)


def test_attention_reference_causal_masking():
    q = torch.randn(1, 1, 8, 4)
    k = torch.randn(1, 1, 8, 4)
    v = torch.randn(1, 1, 8, 4)
    out_full = R.attention(q, k, v, causal=True)
    # first position can only attend to itself
    want0 = v[0, 0, 0]
    torch.testing.assert_close(out_full[0, 0, 0], want0, rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------
# Stochastic rounding and the block-quantised AdamW reference
# ---------------------------------------------------------------------------

def _rnd_hash_int(idx: int, seed: int) -> int:
    """rnd_hash of the lean kernels on plain Python ints."""
    m32 = 0xFFFFFFFF
    x = (((idx ^ (idx >> 31)) & m32) * 0x9E3779B9 + (seed & m32)) & m32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & m32
    return x ^ (x >> 13)


def test_rnd_hash_matches_python_ints():
    g = torch.Generator().manual_seed(3)
    idx = torch.cat([
        torch.arange(0, 70),
        torch.tensor([2 ** 22 - 1, 2 ** 22, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1,
                      2 ** 32, 2 ** 32 + 12345, 2 ** 40 + 7]),
        torch.randint(0, 2 ** 33, (200,), generator=g),
    ])
    for seed in (0, 12345, 0xFFFFFFFF, 2 ** 32 + 5):
        got = R.rnd_hash(idx, seed)
        want = [_rnd_hash_int(int(i), seed) for i in idx]
        assert got.tolist() == want
        assert int(got.min()) >= 0 and int(got.max()) <= 0xFFFFFFFF


def test_f2bf_sr_truncates_dithered_bits():
    f = torch.tensor([1.0, 1.00390625, -1.00390625, 3.0e38, float("inf"),
                      float("nan"), 0.0])
    # 1.00390625 = 1 + 2**-8 sits half way between two bf16 values
    lo = R.f2bf_sr(f, torch.zeros(7, dtype=torch.long))
    hi = R.f2bf_sr(f, torch.full((7,), 0xABCDFFFF, dtype=torch.long))
    assert lo[:3].float().tolist() == [1.0, 1.0, -1.0]
    assert hi[:3].float().tolist() == [1.0, 1.0078125, -1.0078125]
    assert lo[4].item() == float("inf") and hi[4].item() == float("inf")
    assert torch.isnan(lo[5]) and torch.isnan(hi[5])
    assert lo[6].item() == 0.0 and hi[6].item() == 0.0
    # a dither below the remainder's complement never rounds up
    assert R.f2bf_sr(f[1:2], torch.tensor([0x7FFF])).item() == 1.0
    assert R.f2bf_sr(f[1:2], torch.tensor([0x8000])).item() == 1.0078125


def test_nesterov_bf16_step_rounds_up_a_quarter_of_the_time():
    """For a uniform fractional part P(SR != RNE) = E[min(f, 1-f)] = 0.25, and
    every result is one of the two bf16 neighbours of t."""
    g = torch.Generator().manual_seed(4)
    n = 300_007
    theta = torch.randn(n, generator=g).bfloat16()
    mom = (0.1 * torch.randn(n, generator=g)).bfloat16()
    delta = (0.01 * torch.randn(n, generator=g)).bfloat16()
    t, m, th = R.nesterov_bf16_step(theta, delta, mom, 0.7, 0.9, 12345)
    m64 = 0.9 * mom.double() + delta.double()
    t64 = theta.double() + 0.7 * (0.9 * m64 + delta.double())
    torch.testing.assert_close(m.double(), m64, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(t.double(), t64, rtol=1e-6, atol=1e-7)
    ulp = torch.ldexp(torch.ones(n), torch.frexp(t)[1] - 8)  # one bf16 ulp of t
    assert bool(((th.float() - t).abs() < ulp).all())
    share = (th != t.bfloat16()).float().mean().item()
    assert 0.22 <= share <= 0.28, share
    # another seed makes other decisions
    th2 = R.nesterov_bf16_step(theta, delta, mom, 0.7, 0.9, 12346)[2]
    assert (th2 != th).float().mean().item() > 0.2


def _adamw8_state(n, seed):
    g = torch.Generator().manual_seed(seed)
    nb = (n + R.QBLOCK - 1) // R.QBLOCK
    master = torch.randn(n, generator=g)
    grad = (0.1 * torch.randn(n, generator=g)).bfloat16()
    m8 = torch.randint(0, 255, (n,), generator=g).to(torch.uint8)
    v8 = torch.randint(0, 256, (n,), generator=g).to(torch.uint8)
    ms = torch.rand(nb, generator=g) * 1e-3 + 1e-4
    vs = torch.rand(nb, generator=g) * 1e-3 + 1e-4
    return master, grad, m8, v8, ms, vs


def test_adamw8_step_is_adamw_on_the_dequantised_state():
    n = 2 * R.QBLOCK + 901
    master, grad, m8, v8, ms, vs = _adamw8_state(n, 5)
    hp = dict(lr=1e-2, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.1, step=3)
    w, m, sv, m8n, v8n, msn, vsn = R.adamw8_step(master, grad, m8, v8, ms, vs, **hp)
    ref_w = master.clone()
    ref_m = (m8.float() - 127.0) * ms.repeat_interleave(R.QBLOCK)[:n]
    ref_v = (v8.float() * vs.repeat_interleave(R.QBLOCK)[:n]) ** 2
    m_term = max(ref_m.abs().max().item(), grad.float().abs().max().item())
    R.adamw_step(ref_w, torch.empty(n, dtype=torch.bfloat16), grad, ref_m, ref_v, **hp)
    # both compute w*(1 - lr*wd) - update in fp32 in another order of
    # operations: a few ulps of each term, so a few ulps of the largest update
    # absolutely and rtol on the rest
    upd = (ref_w - master * (1.0 - hp["lr"] * hp["weight_decay"])).abs().max().item()
    torch.testing.assert_close(w, ref_w, rtol=1e-6, atol=4 * 2.0 ** -24 * upd)
    # beta1*m and (1-beta1)*g may cancel: ulps of the larger term, not of m
    torch.testing.assert_close(m, ref_m, rtol=1e-6, atol=2 * 2.0 ** -24 * m_term)
    torch.testing.assert_close(sv * sv, ref_v, rtol=1e-6, atol=1e-12)
    assert master.equal(_adamw8_state(n, 5)[0])  # inputs untouched


def test_adamw8_step_codes_within_half_a_quantum():
    n = 2 * R.QBLOCK + 901
    master, grad, m8, v8, ms, vs = _adamw8_state(n, 6)
    # block 1: zero gradient on the zero state -> the 1e-12 scale floor
    blk = slice(R.QBLOCK, 2 * R.QBLOCK)
    grad[blk] = 0
    m8[blk] = 127
    v8[blk] = 0
    w, m, sv, m8n, v8n, msn, vsn = R.adamw8_step(
        master, grad, m8, v8, ms, vs, lr=1e-2, weight_decay=0.1, step=1)
    assert m8n.dtype == torch.uint8 and v8n.dtype == torch.uint8
    assert msn.shape == ms.shape and vsn.shape == vs.shape
    assert msn[1].item() == pytest.approx(1e-12) and vsn[1].item() == pytest.approx(1e-12)
    assert bool((m8n[blk] == 127).all()) and bool((v8n[blk] == 0).all())
    torch.testing.assert_close(msn[[0, 2]], R.block_absmax(m)[[0, 2]] / 127)
    torch.testing.assert_close(vsn[[0, 2]], R.block_absmax(sv)[[0, 2]] / 255)
    mq = msn.repeat_interleave(R.QBLOCK)[:n]
    vq = vsn.repeat_interleave(R.QBLOCK)[:n]
    slack = 1 + 2.0 ** -16  # fp32 rounding of the quotient before rint
    assert bool((((m8n.float() - 127) * mq - m).abs() <= 0.5 * mq * slack).all())
    assert bool(((v8n.float() * vq - sv).abs() <= 0.5 * vq * slack).all())
    assert int(m8n.max()) <= 254 and int(v8n.max()) == 255
    # each block's extreme element takes the extreme code
    assert set(m8n[: R.QBLOCK].tolist()) & {0, 254}
