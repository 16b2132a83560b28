"""GPU (MI355X) tests of the training kernels past one grid pass, at edge
shapes, against exact references.

tests/test_gpu_kernels.py gives each training kernel one friendly shape. Here
every grid-stride kernel takes a second pass and a ragged tail, the
block-quantised optimizers take a second `blk += gridDim.x` iteration and are
compared with the operation they compute, the row kernels run several loop
iterations and empty stripes, cross-entropy leaves its vector path, and the
backward entry points are checked for what they refuse.

Every reference is fp64 (fp32 where the op is defined by its fp32 arithmetic)
of the same bf16-valued inputs. In a second-pass test the whole output is
compared, and then the slice of flat indices past the first pass on its own by
relative L2 error: a tail left as zeros can pass an atol-dominated elementwise
check."""

import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hypha_amd import _C, ops
    from hypha_amd.ops import reference as R

DEV = "cuda:0"

PASS8 = 2048 * 256 * 8  # elements one pass of an 8-wide grid-stride kernel covers
QPASS = 2048 * 2048  # elements one pass of a block-quantised kernel covers
PASS4 = 2048 * 256 * 4  # one pass of the 4-wide dq cast of the attention backward

N2 = PASS8 + 8 * 77 + 5  # second pass: 77 vector groups and a 5-element scalar tail
ELEM_NS = [N2, 5, 2048]  # ... / the scalar path in one thread / no tail
NQ = QPASS + 2048 + 901  # 2050 quant blocks: two in the second iteration, last partial


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=gen(seed)) * scale


def rand_bf16(*shape, seed, scale=1.0):
    return randn(*shape, seed=seed, scale=scale).bfloat16().to(DEV)


def rel_l2(got, want):
    got, want = got.double().flatten(), want.double().flatten()
    return ((got - want).norm() / want.norm()).item()


def check(name, got, want, rtol, atol, pass_size=None):
    """Whole-output comparison; with pass_size also the second-pass slice."""
    assert got.shape == want.shape, (name, got.shape, want.shape)
    got, want = got.double().flatten().cpu(), want.double().flatten().cpu()
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    err = (got - want).abs().max().item() if got.numel() else 0.0
    print(f"{name}: max abs err {err:.3e}")
    torch.testing.assert_close(got, want, rtol=rtol, atol=atol, msg=lambda m: f"{name}: {m}")
    if pass_size is not None and got.numel() > pass_size:
        rel = rel_l2(got[pass_size:], want[pass_size:])
        print(f"{name}: second-pass slice [{pass_size}:] rel L2 {rel:.3e}")
        assert rel <= rtol, (f"{name}: second-pass slice [{pass_size}:{got.numel()}] "
                             f"rel L2 {rel:.3e} > {rtol}")


def check_exact(name, got, want, pass_size=None):
    assert got.dtype == want.dtype and got.shape == want.shape
    g, w = got.flatten().cpu(), want.flatten().cpu()
    bad = (g.view(torch.int16) != w.view(torch.int16)) if g.dtype == torch.bfloat16 else g != w
    print(f"{name}: {int(bad.sum())} of {g.numel()} differ")
    assert not bad.any(), f"{name}: {int(bad.sum())} elements differ, first at {int(bad.nonzero()[0])}"
    if pass_size is not None and g.numel() > pass_size:
        assert not bad[pass_size:].any(), f"{name}: second-pass slice [{pass_size}:] differs"


# ---------------------------------------------------------------------------
# 1. Elementwise family: second pass and tails
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", ELEM_NS)
def test_adamw_step(n):
    master, m, v = randn(n, seed=1), torch.rand(n, generator=gen(2)) * 0.1, \
        torch.rand(n, generator=gen(3)) * 0.01
    g = randn(n, seed=4).bfloat16()
    hp = dict(lr=1e-2, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.1, step=3)
    gm, gmm, gv = master.to(DEV), m.to(DEV), v.to(DEV)
    gp = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    _C.adamw_step_(gm, gp, g.to(DEV), gmm, gv, hp["lr"], hp["beta1"], hp["beta2"],
                   hp["eps"], hp["weight_decay"], hp["step"])
    cp = torch.zeros(n, dtype=torch.bfloat16)
    R.adamw_step(master, cp, g, m, v, **hp)
    check(f"adamw master n={n}", gm, master, 1e-5, 1e-6, PASS8)
    check(f"adamw m n={n}", gmm, m, 1e-5, 1e-6, PASS8)
    check(f"adamw v n={n}", gv, v, 1e-5, 1e-7, PASS8)
    check(f"adamw param n={n}", gp, master, 1e-2, 1e-2, PASS8)
    check_exact(f"adamw param == bf16(master) n={n}", gp, gm.bfloat16(), PASS8)


@pytest.mark.parametrize("n", ELEM_NS)
def test_nesterov_step(n):
    theta, mom = randn(n, seed=5), randn(n, seed=6, scale=0.1)
    delta = randn(n, seed=7, scale=0.1).bfloat16()
    gt, gm = theta.to(DEV), mom.to(DEV)
    _C.nesterov_step_(gt, delta.to(DEV), gm, 0.7, 0.9)
    R.nesterov_outer_step(theta, delta, mom, lr=0.7, mu=0.9)
    check(f"nesterov theta n={n}", gt, theta, 1e-4, 1e-4, PASS8)
    check(f"nesterov mom n={n}", gm, mom, 1e-4, 1e-4, PASS8)


@pytest.mark.parametrize("n", ELEM_NS)
def test_extract_delta(n):
    a, b = randn(n, seed=8).to(DEV), randn(n, seed=9).to(DEV)
    out = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    _C.extract_delta(a, b, out)
    check_exact(f"extract_delta n={n}", out, (a.cpu() - b.cpu()).bfloat16(), PASS8)


@pytest.mark.parametrize("n", ELEM_NS)
def test_extract_delta_bf16(n):
    a, b = rand_bf16(n, seed=10), rand_bf16(n, seed=11)
    out = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    _C.extract_delta_bf16(a, b, out)
    want = (a.cpu().float() - b.cpu().float()).bfloat16()
    check_exact(f"extract_delta_bf16 n={n}", out, want, PASS8)


def _spiked(n, seed):
    """bf16 N(0, 2) with +-20 and +-90 at the head, in the second pass and in
    the scalar tail (where n has them)."""
    x = randn(n, seed=seed, scale=2.0)
    spikes = torch.tensor([20.0, -20.0, 90.0, -90.0])
    for start in (0, PASS8 + 3, n - 4):
        if 0 <= start and start + 4 <= n:
            x[start:start + 4] = spikes
    return x.bfloat16().to(DEV)


@pytest.mark.parametrize("n", ELEM_NS)
def test_swiglu_bindings(n):
    g, u, d = _spiked(n, 12), _spiked(n, 13).flip(0).contiguous(), rand_bf16(n, seed=14)
    out = _C.swiglu_fwd(g, u)
    dg, du = _C.swiglu_bwd(d, g, u)
    g64, u64, d64 = g.double(), u.double(), d.double()
    s = torch.sigmoid(g64)
    check(f"swiglu fwd n={n}", out, g64 * s * u64, 2e-2, 2e-2, PASS8)
    check(f"swiglu dgate n={n}", dg, d64 * u64 * s * (1 + g64 * (1 - s)), 3e-2, 3e-2, PASS8)
    check(f"swiglu dup n={n}", du, d64 * g64 * s, 3e-2, 3e-2, PASS8)


@pytest.mark.parametrize("n", ELEM_NS)
def test_gelu_bindings(n):
    x, d = _spiked(n, 15), rand_bf16(n, seed=16)
    y = _C.gelu_fwd(x)
    dx = _C.gelu_bwd(d, x)
    x64 = x.double().requires_grad_(True)
    want = F.gelu(x64, approximate="tanh")
    want.backward(d.double())
    check(f"gelu fwd n={n}", y, want.detach(), 2e-2, 2e-2, PASS8)
    check(f"gelu bwd n={n}", dx, x64.grad, 3e-2, 3e-2, PASS8)


@pytest.mark.parametrize("n", ELEM_NS)
def test_grad_norm_sq(n):
    x = randn(n, seed=17)
    x[PASS8:] *= 64.0  # a second pass left out must move the sum by more than rtol
    x = x.bfloat16().to(DEV)
    got = _C.grad_norm_sq(x).item()
    want = x.double().pow(2).sum().item()
    print(f"grad_norm_sq n={n}: rel err {abs(got - want) / want:.3e}")
    assert abs(got - want) <= 1e-3 * want, (got, want)
    if n > PASS8:
        tail = x[PASS8:].double().pow(2).sum().item()
        assert tail > 0.1 * want  # the slice carries weight the bound can see


@pytest.mark.parametrize("n", ELEM_NS)
def test_fp8_extract_delta(n):
    """Exact: the scales are bf16-valued, so e4m3 * scale is exact in fp32 and
    the kernel's result does not depend on whether the compiler fuses the
    multiply into the subtraction."""
    nb = (n + 2047) // 2048
    w8 = torch.randint(0, 256, (n,), generator=gen(18)).to(torch.uint8)
    w8[(w8 & 0x7F) == 0x7F] = 0x3A  # no NaN codes
    ws = (torch.rand(nb, generator=gen(19)) * 0.01 + 1e-4).bfloat16().float()
    theta0 = randn(n, seed=20, scale=0.5).bfloat16()
    out = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    _C.fp8_extract_delta(w8.to(DEV), ws.to(DEV), theta0.to(DEV), out)
    deq = w8.view(torch.float8_e4m3fn).float() * ws.repeat_interleave(2048)[:n]
    check_exact(f"fp8_extract_delta n={n}", out, (deq - theta0.float()).bfloat16(), PASS8)


# ---------------------------------------------------------------------------
# 2. Stochastic rounding: nesterov_bf16_ against its bit-level emulation
# ---------------------------------------------------------------------------

def bf16_ulp(t):
    """One bf16 ulp at the magnitude of the fp32 t."""
    return torch.ldexp(torch.ones_like(t), torch.frexp(t)[1] - 8)


def sr_checks(name, got, t, emu):
    """got bf16 from the kernel, t the fp32 value before rounding, emu the
    emulated stochastic rounding of t."""
    got, t, emu = got.cpu(), t.cpu(), emu.cpu()
    off = ((got.float() - t).abs() / bf16_ulp(t)).max().item()
    miss = (got.view(torch.int16) != emu.view(torch.int16)).float().mean().item()
    up = (got.view(torch.int16) != t.bfloat16().view(torch.int16)).float().mean().item()
    print(f"{name}: max |theta - t| {off:.4f} ulp, share != emulation {miss:.3e}, "
          f"share != RNE {up:.4f}")
    assert off <= 1.0, f"{name}: {off} bf16 ulps from the fp32 value"
    # a condition, not a measurement: one fp32 ulp of t (the kernel fuses
    # multiply-adds) moves ~2e-5 of the results, a wrong index or seed tens of %
    assert miss <= 1e-3, f"{name}: share {miss} differs from the emulation"
    return up


@pytest.mark.parametrize("n", ELEM_NS)
def test_nesterov_bf16(n):
    lr, mu, seed = 0.7, 0.9, 12345
    theta = randn(n, seed=21).bfloat16()
    mom = randn(n, seed=22, scale=0.1).bfloat16()
    delta = randn(n, seed=23, scale=0.01).bfloat16()
    gt, gm = theta.to(DEV), mom.to(DEV)
    _C.nesterov_bf16_(gt, delta.to(DEV), gm, lr, mu, seed)
    t, m, emu = R.nesterov_bf16_step(theta, delta, mom, lr, mu, seed)
    mu32 = torch.tensor(mu, dtype=torch.float32).double()
    m64 = mu32 * mom.double() + delta.double()
    # round-to-nearest half ulp; not bit for bit, the kernel's fused
    # multiply-add rounds once where torch rounds twice
    err = (gm.cpu().double() - m64).abs()
    print(f"nesterov_bf16 n={n}: max mom err / |m| {(err / m64.abs()).max().item():.3e}")
    assert bool((err <= 2.0 ** -8 * m64.abs() * 1.01).all())
    up = sr_checks(f"nesterov_bf16 n={n}", gt, t, emu)
    if n > PASS8:
        # P(SR != RNE) = E[min(f, 1-f)] = 0.25 for a uniform fractional part
        assert 0.22 <= up <= 0.28, up
        bad = gt.cpu().view(torch.int16)[PASS8:] != emu.view(torch.int16)[PASS8:]
        # 621 elements: the 1e-3 cap leaves room for none, a wrong index or seed
        # changes a quarter of them; allow the one an fp32 ulp of t may move
        assert int(bad.sum()) <= 1, "second-pass slice differs from the emulation"
        assert bool((err[PASS8:] <= 2.0 ** -8 * m64.abs()[PASS8:] * 1.01).all())


# ---------------------------------------------------------------------------
# 3. Block-quantised optimizers: one step from a random quantised state
# ---------------------------------------------------------------------------

HP8 = dict(lr=1e-2, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.1, step=3)
ZERO_BLK = 7  # zero gradient on the zero state: the 1e-12 scale floor
SEED8 = 424242


@functools.lru_cache(maxsize=None)
def q_state():
    """The shared random quantised state (CPU): grad, m8, v8 and scales."""
    n, nb = NQ, (NQ + 2047) // 2048
    grad = randn(n, seed=30, scale=0.1).bfloat16()
    m8 = torch.randint(0, 255, (n,), generator=gen(31)).to(torch.uint8)
    v8 = torch.randint(0, 256, (n,), generator=gen(32)).to(torch.uint8)
    ms = torch.rand(nb, generator=gen(33)) * 1e-3 + 1e-4
    vs = torch.rand(nb, generator=gen(34)) * 1e-3 + 1e-4
    blk = slice(ZERO_BLK * 2048, (ZERO_BLK + 1) * 2048)
    grad[blk], m8[blk], v8[blk] = 0, 127, 0
    return grad, m8, v8, ms, vs


def q_reference(weight):
    grad, m8, v8, ms, vs = q_state()
    return R.adamw8_step(weight, grad, m8, v8, ms, vs, **HP8)


def q_args():
    return [t.to(DEV) for t in q_state()]


def q_hp():
    return [HP8[k] for k in ("lr", "beta1", "beta2", "eps", "weight_decay", "step")]


def state_checks(name, got, ref):
    """m8, v8 and the scales after one step against the emulation; the blocks
    of the second loop iteration also on their own."""
    gm8, gv8, gms, gvs = (t.cpu() for t in got)
    _, _, _, m8n, v8n, msn, vsn = ref
    for tag, sl, bl in (("all", slice(None), slice(None)),
                        ("second-iteration blocks", slice(QPASS, None), slice(2048, None))):
        for what, g, w in (("m_scale", gms[bl], msn[bl]), ("v_scale", gvs[bl], vsn[bl])):
            rel = ((g - w).abs() / w).max().item()
            print(f"{name} {what} [{tag}]: max rel err {rel:.3e}")
            assert rel <= 1e-6, f"{name}: {what} [{tag}] rel err {rel}"
        for what, g, w in (("m8", gm8[sl], m8n[sl]), ("v8", gv8[sl], v8n[sl])):
            d = (g.int() - w.int()).abs()
            share = (d != 0).float().mean().item()
            print(f"{name} {what} [{tag}]: max code diff {int(d.max())}, share {share:.3e}")
            assert int(d.max()) <= 1, f"{name}: {what} [{tag}] differs by {int(d.max())}"
            assert share <= 1e-3, f"{name}: {what} [{tag}] share {share}"
    assert gms[ZERO_BLK].item() == msn[ZERO_BLK].item() == pytest.approx(1e-12)
    assert gvs[ZERO_BLK].item() == vsn[ZERO_BLK].item() == pytest.approx(1e-12)
    blk = slice(ZERO_BLK * 2048, (ZERO_BLK + 1) * 2048)
    assert bool((gm8[blk] == 127).all()) and bool((gv8[blk] == 0).all())


def test_adamw8_step_one_step():
    master = randn(NQ, seed=35)
    ref = q_reference(master)
    grad, m8, v8, ms, vs = q_args()
    gmaster = master.to(DEV)
    param = torch.zeros(NQ, dtype=torch.bfloat16, device=DEV)
    _C.adamw8_step_(gmaster, param, grad, m8, v8, ms, vs, *q_hp())
    check("adamw8 master", gmaster, ref[0], 1e-5, 1e-6, QPASS)
    check_exact("adamw8 param == bf16(master)", param, gmaster.bfloat16(), QPASS)
    state_checks("adamw8", (m8, v8, ms, vs), ref)


def test_adamw8_lean_one_step():
    p0 = randn(NQ, seed=36).bfloat16()
    ref = q_reference(p0.float())
    grad, m8, v8, ms, vs = q_args()
    param = p0.to(DEV)
    _C.adamw8_lean_(param, grad, m8, v8, ms, vs, *q_hp(), SEED8)
    state_checks("adamw8_lean", (m8, v8, ms, vs), ref)
    w = ref[0]
    emu = R.f2bf_sr(w, R.rnd_hash(torch.arange(NQ), SEED8))
    sr_checks("adamw8_lean param", param, w, emu)
    sr_checks("adamw8_lean param [second-iteration blocks]", param[QPASS:], w[QPASS:],
              emu[QPASS:])


def e4m3(bytes_):
    return bytes_.cpu().view(torch.float8_e4m3fn).float()


def fp8_weight_checks(name, w8, wscale, w):
    """New block scale amax/448, every dequantised weight within one e4m3
    quantum (normal or subnormal) of the fp32 w, no NaN code."""
    w8, wscale = w8.cpu(), wscale.cpu()
    n = w.numel()
    amax = R.block_absmax(w)
    want = torch.where(amax > 0, amax / 448.0, torch.full_like(amax, 1e-12))
    for tag, sl, bl in (("all", slice(None), slice(None)),
                        ("second-iteration blocks", slice(QPASS, None), slice(2048, None))):
        rel = ((wscale[bl] - want[bl]).abs() / want[bl]).max().item()
        print(f"{name} wscale [{tag}]: max rel err {rel:.3e}")
        assert rel <= 1e-6, f"{name}: wscale [{tag}] rel err {rel}"
        sc = wscale.repeat_interleave(2048)[:n][sl]
        err = (e4m3(w8)[sl] * sc - w[sl]).abs()
        bound = 2.0 ** -3 * w[sl].abs() + 2.0 ** -9 * sc
        print(f"{name} [{tag}]: max err / bound {(err / bound).max().item():.4f}")
        assert bool((err <= bound).all()), f"{name}: [{tag}] more than one e4m3 quantum off"
        assert not bool(((w8[sl] & 0x7F) == 0x7F).any()), f"{name}: [{tag}] NaN code stored"


def test_adamw8_fp8_lean_one_step():
    nb = (NQ + 2047) // 2048
    w8 = torch.randint(0, 256, (NQ,), generator=gen(37)).to(torch.uint8)
    w8[(w8 & 0x7F) == 0x7F] = 0x3A
    ws = torch.rand(nb, generator=gen(38)) * 1e-2 + 1e-3
    w_in = e4m3(w8) * ws.repeat_interleave(2048)[:NQ]
    ref = q_reference(w_in)
    grad, m8, v8, ms, vs = q_args()
    gw8, gws = w8.to(DEV), ws.to(DEV)
    _C.adamw8_fp8_lean_(gw8, gws, grad, m8, v8, ms, vs, *q_hp(), SEED8)
    state_checks("adamw8_fp8_lean", (m8, v8, ms, vs), ref)
    fp8_weight_checks("adamw8_fp8_lean", gw8, gws, ref[0])


def test_fp8_requant():
    theta = randn(NQ, seed=39).bfloat16()
    theta[ZERO_BLK * 2048:(ZERO_BLK + 1) * 2048] = 0
    nb = (NQ + 2047) // 2048
    w8 = torch.full((NQ,), 0x7F, dtype=torch.uint8, device=DEV)  # poisoned
    ws = torch.full((nb,), float("nan"), device=DEV)
    _C.fp8_requant_(theta.to(DEV), w8, ws, SEED8)
    fp8_weight_checks("fp8_requant", w8, ws, theta.float())
    assert ws[ZERO_BLK].item() == pytest.approx(1e-12)
    assert bool((w8[ZERO_BLK * 2048:(ZERO_BLK + 1) * 2048] == 0).all())


# ---------------------------------------------------------------------------
# 4. Row kernels: RMSNorm, add+RMSNorm, LayerNorm
# ---------------------------------------------------------------------------

ROW_SHAPES = [(1, 8), (17, 2056), (1000, 776), (1100, 64), (2, 16384)]
EPS = 1e-5


def row_inputs(N, D, seed, zero_mean=False, offset=0.0):
    x = randn(N, D, seed=seed)
    if zero_mean:
        x = x - x.mean(-1, keepdim=True)
    x = (x + offset).bfloat16().to(DEV)
    w = (randn(D, seed=seed + 1, scale=0.1) + 1.0).bfloat16().to(DEV)
    b = randn(D, seed=seed + 2, scale=0.1).bfloat16().to(DEV)
    dy = rand_bf16(N, D, seed=seed + 3)
    return x, w, b, dy


def rms64(x, w):
    x = x.double()
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS)
    return x * rstd * w.double(), rstd.squeeze(-1)


def stat_check(name, got, want, D, scale=None):
    """fp32 row statistic against fp64: rtol = max(D, 64) * 2**-23, the
    worst-case fp32 summation bound plus the rsqrtf ulps. For a sum that may
    cancel (the mean of a zero-mean row) the summation bound is relative to
    sum |x_i| / D, passed as scale, not to the result."""
    rtol = max(D, 64) * 2.0 ** -23
    ref = want.abs() if scale is None else scale
    rel = ((got.double() - want).abs() / ref).max().item()
    print(f"{name}: max rel err {rel:.3e} (bound {rtol:.3e})")
    assert rel <= rtol, f"{name}: {rel} > {rtol}"


def colsum_check(name, got, terms):
    """fp32 column reduction before any bf16 cast against the fp64 sum of the
    same terms: |got - want| <= N * 2**-23 * sum_i |a_i| per column."""
    N = terms.shape[0]
    err = (got.double() - terms.sum(0)).abs()
    bound = N * 2.0 ** -23 * terms.abs().sum(0)
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{name}: max err / bound {worst:.4f}")
    assert bool((err <= bound).all()), f"{name}: {worst} times the summation bound"


@pytest.mark.parametrize("N,D", ROW_SHAPES)
def test_rmsnorm_rows(N, D):
    x, w, _, dy = row_inputs(N, D, seed=40)
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = ops.rmsnorm(xg, wg, EPS)
    y.backward(dy)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    want = rms64(x64, w64)[0]
    want.backward(dy.double())
    tag = f"rmsnorm ({N},{D})"
    check(f"{tag} y", y.detach(), want.detach(), 2e-2, 2e-2)
    check(f"{tag} dx", xg.grad, x64.grad, 3e-2, 3e-2)
    check(f"{tag} dw", wg.grad, w64.grad, 3e-2, 3e-1)


@pytest.mark.parametrize("N,D", ROW_SHAPES)
def test_rmsnorm_stats_and_dw(N, D):
    x, w, _, dy = row_inputs(N, D, seed=44, zero_mean=True)
    y, rstd = _C.rmsnorm_fwd(x, w, EPS)
    dx, dw = _C.rmsnorm_bwd(dy, x, w, rstd)
    assert rstd.dtype == torch.float32 and dw.dtype == torch.float32
    tag = f"rmsnorm ({N},{D})"
    stat_check(f"{tag} rstd", rstd, rms64(x, w)[1], D)
    colsum_check(f"{tag} fp32 dw", dw, dy.double() * x.double() * rstd.double()[:, None])


@pytest.mark.parametrize("N,D", ROW_SHAPES)
def test_add_rmsnorm_rows(N, D):
    a, w, _, dy = row_inputs(N, D, seed=48)
    b, dh = rand_bf16(N, D, seed=52), rand_bf16(N, D, seed=53)
    ag, bg, wg = (t.clone().requires_grad_(True) for t in (a, b, w))
    h, y = ops.add_rmsnorm(ag, bg, wg, EPS)
    torch.autograd.backward([h, y], [dh, dy])
    a64, b64, w64 = (t.double().requires_grad_(True) for t in (a, b, w))
    h64 = a64 + b64
    y64 = rms64(h64, w64)[0]
    torch.autograd.backward([h64, y64], [dh.double(), dy.double()])
    tag = f"add_rmsnorm ({N},{D})"
    check(f"{tag} h", h.detach(), h64.detach(), 2e-2, 2e-2)
    check(f"{tag} y", y.detach(), y64.detach(), 2e-2, 2e-2)
    check(f"{tag} da", ag.grad, a64.grad, 3e-2, 3e-2)
    check(f"{tag} db", bg.grad, b64.grad, 3e-2, 3e-2)
    check(f"{tag} dw", wg.grad, w64.grad, 3e-2, 3e-1)


@pytest.mark.parametrize("N,D", ROW_SHAPES)
def test_add_rmsnorm_stats_and_dw(N, D):
    a, w, _, dy = row_inputs(N, D, seed=54, zero_mean=True)
    b = row_inputs(N, D, seed=58, zero_mean=True)[0]
    dh = rand_bf16(N, D, seed=62)
    h, y, rstd = _C.add_rmsnorm_fwd(a, b, w, EPS)
    dx, dw = _C.add_rmsnorm_bwd(dy, dh, h, w, rstd)
    assert rstd.dtype == torch.float32 and dw.dtype == torch.float32
    tag = f"add_rmsnorm ({N},{D})"
    stat_check(f"{tag} rstd", rstd, rms64(a.double() + b.double(), w)[1], D)
    colsum_check(f"{tag} fp32 dw", dw, dy.double() * h.double() * rstd.double()[:, None])
    # without the residual gradient the wrapper takes rmsnorm_bwd on h
    dx2, dw2 = _C.rmsnorm_bwd(dy, h, w, rstd)
    colsum_check(f"{tag} fp32 dw (no dh)", dw2, dy.double() * h.double() * rstd.double()[:, None])


def ln64(x, w, b):
    return F.layer_norm(x, (x.shape[-1],), w, b, EPS)


@pytest.mark.parametrize("N,D", ROW_SHAPES)
def test_layernorm_rows(N, D):
    x, w, b, dy = row_inputs(N, D, seed=63)
    xg, wg, bg = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = ops.layernorm(xg, wg, bg, EPS)
    y.backward(dy)
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    want = ln64(x64, w64, b64)
    want.backward(dy.double())
    tag = f"layernorm ({N},{D})"
    check(f"{tag} y", y.detach(), want.detach(), 2e-2, 2e-2)
    check(f"{tag} dx", xg.grad, x64.grad, 3e-2, 3e-2)
    check(f"{tag} dw", wg.grad, w64.grad, 3e-2, 3e-1)
    check(f"{tag} db", bg.grad, b64.grad, 3e-2, 3e-1)


@pytest.mark.parametrize("N,D", ROW_SHAPES)
def test_layernorm_stats_and_dwdb(N, D):
    x, w, b, dy = row_inputs(N, D, seed=67, zero_mean=True)
    y, mean, rstd = _C.layernorm_fwd(x, w, b, EPS)
    dx, dw, db = _C.layernorm_bwd(dy, x, w, mean, rstd)
    assert mean.dtype == rstd.dtype == dw.dtype == db.dtype == torch.float32
    x64 = x.double()
    tag = f"layernorm ({N},{D})"
    stat_check(f"{tag} mean", mean, x64.mean(-1), D, scale=x64.abs().mean(-1))
    stat_check(f"{tag} rstd", rstd, torch.rsqrt(x64.var(-1, unbiased=False) + EPS), D)
    xhat = (x64 - mean.double()[:, None]) * rstd.double()[:, None]
    colsum_check(f"{tag} fp32 dw", dw, dy.double() * xhat)
    colsum_check(f"{tag} fp32 db", db, dy.double())


def test_layernorm_offset_rows():
    """Rows of mean 100, std 1: E[x^2] - mean^2 cancels four digits, which
    bf16 inputs (ulp 0.5 at 100) leave room for in fp32."""
    N, D = 17, 2056
    x, w, b, _ = row_inputs(N, D, seed=71, offset=100.0)
    y = ops.layernorm(x, w, b, EPS)
    check("layernorm +100", y, ln64(x.double(), w.double(), b.double()), 2e-2, 2e-2)


def test_rmsnorm_backward_of_sum():
    """loss = y.sum() hands the wrapper a stride-0 dy."""
    N, D = 17, 2056
    x, w, _, _ = row_inputs(N, D, seed=75)
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    ops.rmsnorm(xg, wg, EPS).sum().backward()
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    rms64(x64, w64)[0].sum().backward()
    check("rmsnorm sum dx", xg.grad, x64.grad, 3e-2, 3e-2)
    check("rmsnorm sum dw", wg.grad, w64.grad, 3e-2, 3e-1)


def test_add_rmsnorm_refuses_d_over_limit():
    a, b = rand_bf16(2, 16392, seed=76), rand_bf16(2, 16392, seed=77)
    w = torch.ones(16392, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        ops.add_rmsnorm(a, b, w, EPS)


# ---------------------------------------------------------------------------
# 5. Cross-entropy
# ---------------------------------------------------------------------------

CE_SHAPES = [(5, 7), (33, 1003), (4, 4107), (3, 50257)]


def ce_checks(tag, logits, targets):
    """lse, mean loss and dlogits of one batch against fp64."""
    N, V = logits.shape
    l64 = logits.double()
    tg = targets.to(DEV)
    valid = tg >= 0
    n_valid = int(valid.sum())
    lse64 = torch.logsumexp(l64, -1)
    lse_bound = V * 2.0 ** -23 + 1e-5
    _, lse, nv = _C.ce_fwd(logits, tg)
    lse_err = (lse.double() - lse64).abs().max().item()
    print(f"{tag}: max lse err {lse_err:.3e} (bound {lse_bound:.3e})")
    assert lse.dtype == torch.float32 and int(nv) == n_valid
    assert lse_err <= lse_bound, f"{tag}: lse err {lse_err} > {lse_bound}"

    lg = logits.clone().requires_grad_(True)  # the backward overwrites it
    loss = ops.cross_entropy_loss(lg, tg)
    l64g = l64.clone().requires_grad_(True)
    if n_valid:
        want = F.cross_entropy(l64g, tg, ignore_index=-100)
        want.backward()
        want, wgrad = want.item(), l64g.grad
    else:
        want, wgrad = 0.0, torch.zeros_like(l64)
    loss_bound = 2 * lse_bound + N * 2.0 ** -23 * abs(want)
    print(f"{tag}: loss err {abs(loss.item() - want):.3e} (bound {loss_bound:.3e})")
    assert abs(loss.item() - want) <= loss_bound, (tag, loss.item(), want)
    loss.backward()
    check(f"{tag} dlogits", lg.grad, wgrad, 5e-2, 1e-4)
    ignored = lg.grad[~valid]
    assert bool((ignored == 0).all()), f"{tag}: ignored rows not exactly zero"
    return loss


@pytest.mark.parametrize("N,V", CE_SHAPES)
def test_ce_targets(N, V):
    """Targets at index 0, at V-1 (the scalar tail where V % 8 != 0), in the
    second loop iteration's vector part where V has one, and ignored."""
    logits = rand_bf16(N, V, seed=80, scale=3.0)
    kinds = [0, V - 1, 2050 if V > 2058 else V // 2, -100]
    for r in (0, 1):  # two rotations put every kind on a row even at N = 3
        t = torch.tensor([kinds[(r + i) % 4] for i in range(N)])
        ce_checks(f"ce ({N},{V}) rotation {r}", logits, t)


@pytest.mark.parametrize("N,V", CE_SHAPES)
def test_ce_rows(N, V):
    """A random row, a row with one logit +80 among -80 (the +80 last, in the
    scalar tail: at large V it is the one logit whose loss the lse bound cannot
    miss), a row of equal logits."""
    x = randn(N, V, seed=81, scale=3.0)
    x[1] = -80.0
    x[1, V - 1] = 80.0
    x[2] = 3.0
    t = torch.randint(0, V, (N,), generator=gen(82))
    t[1] = 0  # loss 160 on the peaked row
    ce_checks(f"ce rows ({N},{V})", x.bfloat16().to(DEV), t)


@pytest.mark.parametrize("N,V", CE_SHAPES)
def test_ce_all_ignored(N, V):
    logits = rand_bf16(N, V, seed=83, scale=3.0)
    lg = logits.clone().requires_grad_(True)
    loss = ops.cross_entropy_loss(lg, torch.full((N,), -100, device=DEV))
    assert loss.item() == 0.0
    loss.backward()
    assert bool((lg.grad == 0).all())
    ce_checks(f"ce all ignored ({N},{V})", logits, torch.full((N,), -100))


# ---------------------------------------------------------------------------
# 6. RoPE
# ---------------------------------------------------------------------------

def rope_case(qshape, kshape, layout, table_len, pass_size=None):
    D = qshape[-1]
    cos, sin = R.rope_cos_sin(table_len, D, base=10000.0)
    cosg, sing = cos.to(DEV), sin.to(DEV)
    q, k = rand_bf16(*qshape, seed=90), rand_bf16(*kshape, seed=91)
    dqo, dko = rand_bf16(*qshape, seed=92), rand_bf16(*kshape, seed=93)
    qg, kg = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    qo, ko = ops.apply_rope_qk(qg, kg, cosg, sing, layout=layout)
    torch.autograd.backward([qo, ko], [dqo, dko])

    def to_bhsd(t):
        return t.transpose(1, 2) if layout == "bshd" else t

    qf, kf = q.float().requires_grad_(True), k.float().requires_grad_(True)
    qw = to_bhsd(R.apply_rope(to_bhsd(qf), cosg, sing))
    kw = to_bhsd(R.apply_rope(to_bhsd(kf), cosg, sing))
    torch.autograd.backward([qw, kw], [dqo.float(), dko.float()])
    tag = f"rope {layout} {tuple(qshape)}"
    check(f"{tag} q", qo.detach(), qw.detach(), 2e-2, 2e-2, pass_size)
    check(f"{tag} k", ko.detach(), kw.detach(), 2e-2, 2e-2)
    check(f"{tag} dq", qg.grad, qf.grad, 3e-2, 3e-2, pass_size)
    check(f"{tag} dk", kg.grad, kf.grad, 3e-2, 3e-2)


def test_rope_second_pass():
    """q has 655,360 work items of 4 pairs, above the 524,288 of one pass; the
    items past the first pass are the flat elements from PASS8 on."""
    assert 40 * 1024 * (128 // 8) > 2048 * 256
    rope_case((1, 40, 1024, 128), (1, 8, 1024, 128), "bhsd", 1024, pass_size=PASS8)


def test_rope_bshd_long_table():
    rope_case((2, 130, 3, 64), (2, 130, 1, 64), "bshd", 2048)


# ---------------------------------------------------------------------------
# 7. Attention forward and backward
# ---------------------------------------------------------------------------

def attention64(q, k, v, causal):
    """fp64 attention on bhsd tensors; returns (o, lse)."""
    S, D = q.shape[2], q.shape[3]
    rep = q.shape[1] // k.shape[1]
    kk, vv = k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1)
    scores = q @ kk.transpose(-1, -2) / math.sqrt(D)
    if causal:
        mask = torch.ones(S, S, dtype=torch.bool, device=q.device).tril()
        scores = scores.masked_fill(~mask, float("-inf"))
    return torch.softmax(scores, -1) @ vv, torch.logsumexp(scores, -1)


@pytest.mark.parametrize("B,Hq,Hkv,S,D,causal,layout", [
    (1, 2, 2, 128, 64, True, "bhsd"),  # one tile
    (1, 8, 1, 384, 64, True, "bhsd"),  # GQA 8 at D=64, three tiles
    (1, 8, 1, 384, 64, False, "bhsd"),
    (1, 8, 1, 384, 64, True, "bshd"),
    (1, 8, 2, 2176, 128, True, "bhsd"),  # dq past one pass of its bf16 cast
])
def test_attention_edges(B, Hq, Hkv, S, D, causal, layout):
    q, do = rand_bf16(B, Hq, S, D, seed=100), rand_bf16(B, Hq, S, D, seed=103)
    k, v = rand_bf16(B, Hkv, S, D, seed=101), rand_bf16(B, Hkv, S, D, seed=102)

    def lay(t):  # bhsd -> the kernel's layout and back (its own inverse)
        return t.transpose(1, 2).contiguous() if layout == "bshd" else t

    o, lse = _C.attn_fwd_ex(lay(q), lay(k), lay(v), causal, layout)
    dq, dk, dv = _C.attn_bwd_ex(lay(q), lay(k), lay(v), o, lay(do), lse, causal, layout)
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    o64, lse64 = attention64(q64, k64, v64, causal)
    o64.backward(do.double())
    tag = f"attention ({B},{Hq},{Hkv},{S},{D}) causal={causal} {layout}"
    assert lse.shape == (B, Hq, S) and lse.dtype == torch.float32
    check(f"{tag} o", lay(o), o64.detach(), 2e-2, 2e-2)
    check(f"{tag} lse", lse, lse64.detach(), 2e-2, 2e-2)
    n_dq = dq.numel()
    assert (n_dq > PASS4) == (S == 2176)
    check(f"{tag} dq", lay(dq), q64.grad, 5e-2, 5e-2, PASS4 if n_dq > PASS4 else None)
    check(f"{tag} dk", lay(dk), k64.grad, 5e-2, 5e-2)
    check(f"{tag} dv", lay(dv), v64.grad, 5e-2, 5e-2)


# ---------------------------------------------------------------------------
# 8. Grouped GEMM, fp8_scale_update_, argument checks, empty inputs
# ---------------------------------------------------------------------------

def test_grouped_gemm_single_k_step():
    """K = 32 is one k-step (the prefetch branch is never taken); counts cross
    a row tile by one, hold one row, and end on an empty group."""
    K, N, counts = 32, 128, [128, 129, 1, 0]
    T = sum(counts)
    x, w = rand_bf16(T, K, seed=110), rand_bf16(len(counts), N, K, seed=111, scale=0.1)
    off = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32)
    got = _C.grouped_gemm(x, w, off)
    want = torch.cat([x[a:b].double() @ w[g].double().t()
                      for g, (a, b) in enumerate(zip(off[:-1].tolist(), off[1:].tolist()))])
    check("grouped_gemm K=32", got, want, 3e-2, 3e-2)


def test_grouped_gemm_all_groups_empty():
    x = torch.empty(0, 32, dtype=torch.bfloat16, device=DEV)
    w = rand_bf16(4, 128, 32, seed=112)
    got = _C.grouped_gemm(x, w, torch.zeros(5, dtype=torch.int32))
    assert got.shape == (0, 128) and got.dtype == torch.bfloat16


def test_fp8_scale_update():
    margin = 1.25
    f32 = torch.float32

    def want(amax):
        return (torch.tensor(amax, dtype=f32) / 448.0 * margin).item()

    scale = torch.zeros(1, device=DEV)
    p = torch.rand(1000, generator=gen(113)).to(DEV)
    p[777] = 5.5  # above the 256 threads' first loads
    _C.fp8_scale_update_(p, scale, margin, 1000)
    assert scale.item() == pytest.approx(want(5.5), rel=1e-6)
    _C.fp8_scale_update_(p, scale, margin)  # n = 0: all of partials
    assert scale.item() == pytest.approx(want(5.5), rel=1e-6)
    p[900] = 9.0  # stale, beyond n
    _C.fp8_scale_update_(p, scale, margin, 800)
    assert scale.item() == pytest.approx(want(5.5), rel=1e-6)
    _C.fp8_scale_update_(torch.zeros(1000, device=DEV), scale, margin, 1000)
    assert scale.item() == pytest.approx(want(1e-8), rel=1e-6)


def _bad(t, how):
    """A tensor in place of t that a kernel must not be handed."""
    if how == "dtype":
        return t.float() if t.dtype != torch.float32 else t.bfloat16()
    if how == "strided":  # t's shape, not contiguous
        return torch.cat([t, t], -1)[..., ::2]
    if how == "short":  # one fewer along the first dim: an out-of-bounds read
        return t[:-1].contiguous()
    if how == "half_s":  # 4-D [B, H, S, D] with half the sequence
        return t[:, :, : t.shape[2] // 2].contiguous()
    if how == "half_d":
        return t[..., : t.shape[3] // 2].contiguous()
    if how == "reshaped":  # same numel, another shape
        return t.reshape(t.shape[0] * 2, -1)
    raise AssertionError(how)


def _good_args(fn):
    """Arguments the entry point accepts; fn names the binding."""
    N, D = 16, 64
    x, w, b, dy = row_inputs(N, D, seed=120)
    dh = rand_bf16(N, D, seed=124)
    stat, stat2 = torch.ones(N, device=DEV), torch.zeros(N, device=DEV)
    if fn in ("attn_bwd_ex", "rope_fwd_ex"):
        B, H, S, HD = 1, 2, 128, 64
        q, k, v, o, do = (rand_bf16(B, H, S, HD, seed=130 + i) for i in range(5))
        if fn == "attn_bwd_ex":
            return [q, k, v, o, do, torch.zeros(B, H, S, device=DEV), True, "bhsd"]
        cos, sin = (t.to(DEV) for t in R.rope_cos_sin(S, HD))
        return [q, k, cos, sin, False, "bhsd"]
    return {
        "rmsnorm_bwd": [dy, x, w, stat],
        "add_rmsnorm_bwd": [dy, dh, x, w, stat],
        "layernorm_bwd": [dy, x, w, stat2, stat],
        "swiglu_fwd": [x, dy],
        "swiglu_bwd": [dh, x, dy],
        "gelu_bwd": [dy, x],
        "ce_bwd_": [x, torch.zeros(N, dtype=torch.long, device=DEV), stat, 1.0],
    }[fn]


ROWS3 = ("dtype", "strided", "short")
VEC2 = ("dtype", "short")
BAD_ARGS = [  # binding, argument position and name, what is wrong with it
    ("rmsnorm_bwd", 0, "dy", ROWS3), ("rmsnorm_bwd", 3, "rstd", VEC2),
    ("add_rmsnorm_bwd", 0, "dy", ROWS3), ("add_rmsnorm_bwd", 1, "dh", ROWS3),
    ("add_rmsnorm_bwd", 4, "rstd", VEC2),
    ("layernorm_bwd", 0, "dy", ROWS3), ("layernorm_bwd", 3, "mean", VEC2),
    ("layernorm_bwd", 4, "rstd", VEC2),
    ("swiglu_fwd", 1, "up", ROWS3 + ("reshaped",)),
    ("swiglu_bwd", 0, "dout", ROWS3), ("swiglu_bwd", 2, "up", ROWS3),
    ("gelu_bwd", 0, "dy", ROWS3 + ("reshaped",)),
    ("ce_bwd_", 1, "targets", VEC2), ("ce_bwd_", 2, "lse", VEC2),
    ("attn_bwd_ex", 1, "k", ("dtype", "strided", "half_s", "half_d")),
    ("attn_bwd_ex", 2, "v", ("dtype", "strided", "half_s", "half_d")),
    ("attn_bwd_ex", 3, "o", ("dtype", "strided", "half_s", "half_d")),
    ("attn_bwd_ex", 4, "dout", ("dtype", "strided", "half_s", "half_d")),
    ("attn_bwd_ex", 5, "lse", ("dtype", "strided", "half_s")),
    ("rope_fwd_ex", 1, "k", ("dtype", "strided", "half_s", "half_d")),
    ("rope_fwd_ex", 3, "sin", ROWS3),
]


@pytest.mark.parametrize("fn,pos,how", [
    pytest.param(fn, pos, how, id=f"{fn}-{name}-{how}")
    for fn, pos, name, hows in BAD_ARGS for how in hows])
def test_entry_points_refuse_bad_arguments(fn, pos, how):
    """Each of these checks stands before the entry point's first launch (a
    mis-shaped tensor reaching a kernel is an out-of-bounds access), so no
    kernel runs here."""
    args = _good_args(fn)
    if fn == "attn_bwd_ex" and pos == 5 and how == "half_s":
        args[pos] = args[pos][:, :, :64].contiguous()  # lse is [B, H, S]
    else:
        args[pos] = _bad(args[pos], how)
    with pytest.raises(RuntimeError):
        getattr(_C, fn)(*args)


def test_empty_inputs_launch_nothing():
    """N = 0 returns right-shaped outputs without a zero-sized launch, which
    would leave an error behind for the next call."""
    D = 64
    x = torch.empty(0, D, dtype=torch.bfloat16, device=DEV)
    w = torch.ones(D, dtype=torch.bfloat16, device=DEV)
    stat = torch.empty(0, device=DEV)
    y, rstd = _C.rmsnorm_fwd(x, w, EPS)
    assert y.shape == (0, D) and rstd.shape == (0,)
    dx, dw = _C.rmsnorm_bwd(x, x, w, stat)
    assert dx.shape == (0, D) and dw.shape == (D,) and bool((dw == 0).all())
    h, y, rstd = _C.add_rmsnorm_fwd(x, x, w, EPS)
    assert h.shape == y.shape == (0, D) and rstd.shape == (0,)
    dx, dw = _C.add_rmsnorm_bwd(x, x, x, w, stat)
    assert dx.shape == (0, D) and dw.shape == (D,) and bool((dw == 0).all())
    y, mean, rstd = _C.layernorm_fwd(x, w, w, EPS)
    assert y.shape == (0, D) and mean.shape == rstd.shape == (0,)
    dx, dw, db = _C.layernorm_bwd(x, x, w, stat, stat)
    assert dx.shape == (0, D) and dw.shape == db.shape == (D,)
    assert bool((dw == 0).all()) and bool((db == 0).all())
    tg = torch.empty(0, dtype=torch.long, device=DEV)
    loss, lse, nv = _C.ce_fwd(x, tg)
    assert loss.item() == 0.0 and lse.shape == (0,) and int(nv) == 0
    assert _C.ce_bwd_(x, tg, stat, 1.0).shape == (0, D)
    torch.cuda.synchronize()
    # a normal call straight after is still right
    xs, ws, _, _ = row_inputs(17, D, seed=150)
    y, _ = _C.rmsnorm_fwd(xs, ws, EPS)
    check("rmsnorm after the empty calls", y, rms64(xs, ws)[0], 2e-2, 2e-2)
    assert ops.cross_entropy_loss(x.requires_grad_(True), tg).item() == 0.0
    torch.cuda.synchronize()
