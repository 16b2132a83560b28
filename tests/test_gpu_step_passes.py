"""GPU (MI355X) tests of the training step without its clip, zero, grad-add
and loss-copy passes: the clip coefficient applied inside AdamW, weight
gradients written into the flat gradient buffer by the wgrad GEMM, and the
shifted loss on unsliced logits. Every one is compared with the form it
replaces (HYPHA_STEP_ABLATE restores it in the same build): exactly where that
form reproduces itself, otherwise against fp64 within the former form's own
error."""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hypha_amd import _C, models, ops
    from hypha_amd.data.synthetic import SyntheticTokens
    from hypha_amd.parallel import Comm, DiLoCoConfig, DiLoCoWorker
    from hypha_amd.parallel.diloco import (WgradInplaceLinear,
                                           convert_linears_to_wgrad_inplace, lr_at)

DEV = "cuda:0"
SENTINEL = 1e4  # finite: a GEMM with beta 0 may still multiply what it finds by 0


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def rand_bf16(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=gen(seed)) * scale).bfloat16().to(DEV)


def rel_l2(got, want):
    got, want = got.double().flatten(), want.double().flatten()
    return ((got - want).norm() / want.norm()).item()


# ---------------------------------------------------------------------------
# AdamW with the clip coefficient applied at the gradient load
# ---------------------------------------------------------------------------

HP = dict(lr=3e-3, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.1)
# one full grid pass (2048 blocks x 256 threads x 8) + 3 full groups + 5-element tail
N_BIG = 4_194_304 + 29


def adamw_state(n):
    master = torch.randn(n, generator=gen(1)).to(DEV)
    return [master, master.bfloat16(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]


@pytest.mark.parametrize("coef", [1.0, 0.3, 1e-3])
@pytest.mark.parametrize("n", [1, 7, 8, N_BIG])
def test_adamw_grad_scale_equals_two_pass(n, coef):
    """ops.fused_adamw(grad_scale=c) == grad.mul_(c.to(bf16)); _C.adamw_step_,
    bit for bit on master, param, m and v, over two steps (the second with
    non-zero m and v)."""
    coef_t = torch.tensor(coef, device=DEV)  # fp32; 0.3 is not a bf16 value
    new, old, plain = adamw_state(n), adamw_state(n), adamw_state(n)
    for step in (1, 2):
        grad = rand_bf16(n, seed=10 + step, scale=0.05)
        kept = grad.clone()
        ops.fused_adamw(new[0], new[1], grad, new[2], new[3], step=step,
                        grad_scale=coef_t, **HP)
        assert torch.equal(grad, kept), "grad_scale must not write the gradients"
        two_pass = grad.clone()
        two_pass.mul_(coef_t.to(torch.bfloat16))
        _C.adamw_step_(old[0], old[1], two_pass, old[2], old[3], HP["lr"], HP["beta1"],
                       HP["beta2"], HP["eps"], HP["weight_decay"], step)
        for name, a, b in zip(("master", "param", "m", "v"), new, old):
            assert torch.equal(a, b), (
                f"step {step} {name}: {int((a != b).sum())} of {n} differ from two-pass")
        if coef == 1.0:
            ops.fused_adamw(plain[0], plain[1], grad, plain[2], plain[3], step=step, **HP)
            for name, a, b in zip(("master", "param", "m", "v"), new, plain):
                assert torch.equal(a, b), f"step {step} {name}: coefficient 1 != unclipped"
    assert torch.isfinite(new[0]).all()


# ---------------------------------------------------------------------------
# Linear backward with dw written into the destination
# ---------------------------------------------------------------------------

T, K, N = 96, 128, 64
GUARD = 8  # elements = 16 bytes: the view behind it stays 16-byte aligned


def linear_inputs():
    return (rand_bf16(T, K, seed=21), rand_bf16(N, K, seed=22, scale=0.1),
            rand_bf16(T, N, seed=23))


def stock_backward(xs, w, dys):
    """nn.Linear + autograd on fresh leaves; one term per (x, dy) pair."""
    lin = nn.Linear(K, N, bias=False, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(w)
    xs = [x.clone().requires_grad_() for x in xs]
    torch.autograd.backward([lin(x) for x in xs], dys)
    return [x.grad for x in xs], lin.weight.grad


def inplace_module(w, offset, fill):
    """WgradInplaceLinear whose weight.grad is a view `offset` elements into a
    sentinel buffer, pre-filled with `fill`, guard bands on both sides."""
    lin = nn.Linear(K, N, bias=False, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(w)
    mod = WgradInplaceLinear.from_linear(lin)
    assert mod.weight is lin.weight and list(mod.state_dict()) == ["weight"]
    buf = torch.full((N * K + 4 * GUARD,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    assert buf.data_ptr() % 16 == 0
    dest = buf[offset:offset + N * K].view(N, K)
    dest.fill_(fill)
    mod.weight.grad = dest
    mod.weight._wgrad_fresh = True
    return mod, buf, dest


def guards_intact(buf, offset):
    return bool((buf[:offset] == SENTINEL).all() and (buf[offset + N * K:] == SENTINEL).all())


def compare_with_stock(name, got, stock_fn, ref64):
    """Equal to stock if stock reproduces itself bit for bit; otherwise both
    against fp64, the new path allowed 1.5 x stock's relative L2 error (the
    same GEMM; the margin covers the library's algorithm choice)."""
    a, b = stock_fn(), stock_fn()
    if torch.equal(a, b):
        ndiff = int((got != a).sum())
        print(f"{name}: stock reproduces itself; {ndiff} of {got.numel()} differ")
        assert ndiff == 0, f"{name}: {ndiff} elements differ from stock"
        return
    e_new, e_stock = rel_l2(got, ref64), rel_l2(a, ref64)
    print(f"{name}: rel L2 vs fp64: new {e_new:.3e}, stock {e_stock:.3e}")
    assert e_new <= 1.5 * e_stock, f"{name}: {e_new:.3e} > 1.5 x {e_stock:.3e}"


def test_linear_bwd_overwrites_destination():
    x, w, dy = linear_inputs()
    mod, buf, dest = inplace_module(w, GUARD, SENTINEL)
    assert ops.interface.wgrad_inplace_ok(mod.weight)
    xin = x.clone().requires_grad_()
    y = mod(xin)
    assert torch.equal(y, F.linear(x, w))
    y.backward(dy)
    assert mod.weight.grad.data_ptr() == dest.data_ptr() and mod.weight._wgrad_fresh is False
    assert guards_intact(buf, GUARD)
    assert torch.isfinite(dest).all() and not (dest == SENTINEL).any()
    compare_with_stock("dx", xin.grad, lambda: stock_backward([x], w, [dy])[0][0],
                       dy.double() @ w.double())
    compare_with_stock("dw", dest, lambda: stock_backward([x], w, [dy])[1],
                       dy.double().t() @ x.double())


def test_linear_bwd_second_write_accumulates():
    """The module used twice in one step: the first wgrad overwrites the
    sentinel, the second adds to the first. Bound: the error stock's own
    accumulation (dw1 + dw2 through autograd) makes on the same inputs."""
    x, w, dy = linear_inputs()
    x2, dy2 = rand_bf16(T, K, seed=24), rand_bf16(T, N, seed=25)
    mod, buf, dest = inplace_module(w, GUARD, SENTINEL)
    xa, xb = x.clone().requires_grad_(), x2.clone().requires_grad_()
    torch.autograd.backward([mod(xa), mod(xb)], [dy, dy2])
    assert guards_intact(buf, GUARD)
    ref64 = dy.double().t() @ x.double() + dy2.double().t() @ x2.double()
    (sa, sb), stock_dw = stock_backward([x, x2], w, [dy, dy2])
    e_new, e_stock = rel_l2(dest, ref64), rel_l2(stock_dw, ref64)
    print(f"sum of two dw: rel L2 vs fp64: new {e_new:.3e}, stock {e_stock:.3e}")
    assert e_new <= e_stock, f"accumulated dw: {e_new:.3e} > stock's {e_stock:.3e}"
    compare_with_stock("dx first use", xa.grad,
                       lambda: stock_backward([x, x2], w, [dy, dy2])[0][0],
                       dy.double() @ w.double())
    compare_with_stock("dx second use", xb.grad,
                       lambda: stock_backward([x, x2], w, [dy, dy2])[0][1],
                       dy2.double() @ w.double())


def test_linear_bwd_unaligned_destination_falls_back():
    """A grad view one element off 16-byte alignment: dw comes back through
    autograd, which adds it to the (zeroed) view; nothing else is written."""
    x, w, dy = linear_inputs()
    mod, buf, dest = inplace_module(w, GUARD + 1, 0.0)
    assert dest.data_ptr() % 16 != 0 and not ops.interface.wgrad_inplace_ok(mod.weight)
    xin = x.clone().requires_grad_()
    mod(xin).backward(dy)
    assert mod.weight._wgrad_fresh is True, "the fallback writes nothing in place"
    assert guards_intact(buf, GUARD + 1)
    compare_with_stock("dx", xin.grad, lambda: stock_backward([x], w, [dy])[0][0],
                       dy.double() @ w.double())
    compare_with_stock("dw", mod.weight.grad, lambda: stock_backward([x], w, [dy])[1],
                       dy.double().t() @ x.double())


def test_linear_bwd_without_grad_falls_back():
    x, w, dy = linear_inputs()
    mod, buf, dest = inplace_module(w, GUARD, SENTINEL)
    mod.weight.grad = None
    xin = x.clone().requires_grad_()
    mod(xin).backward(dy)
    assert (buf == SENTINEL).all(), "the detached buffer must stay untouched"
    assert mod.weight.grad is not None and mod.weight.grad.data_ptr() != dest.data_ptr()
    compare_with_stock("dx", xin.grad, lambda: stock_backward([x], w, [dy])[0][0],
                       dy.double() @ w.double())
    compare_with_stock("dw", mod.weight.grad, lambda: stock_backward([x], w, [dy])[1],
                       dy.double().t() @ x.double())


# ---------------------------------------------------------------------------
# Worker level: new path against HYPHA_STEP_ABLATE=7 (the former passes)
# ---------------------------------------------------------------------------


def assert_within_legacy_spread(name, new, legacy_a, legacy_b):
    """Equal if two legacy runs are equal; otherwise within twice their spread."""
    spread = (legacy_a - legacy_b).abs().max().item()
    diff = max((new - legacy_a).abs().max().item(), (new - legacy_b).abs().max().item())
    print(f"{name}: legacy spread {spread:.3e}, new-to-legacy max abs diff {diff:.3e}")
    if spread == 0.0:
        assert torch.equal(new, legacy_a), f"{name}: differs from a reproducible legacy"
    else:
        assert diff <= 2 * spread, f"{name}: {diff:.3e} > 2 x {spread:.3e}"


def run_llama_tiny(monkeypatch, ablate, ckpt):
    monkeypatch.setenv("HYPHA_STEP_ABLATE", str(ablate))
    torch.manual_seed(0)
    model = models.build("llama-tiny", gradient_checkpointing=ckpt)
    worker = DiLoCoWorker(model, DiLoCoConfig(h=100), comm=Comm(),
                          device=torch.device(DEV))
    data = SyntheticTokens(512, 128, 2, seed=5)
    losses = [worker.train_step(*data.next_batch()) for _ in range(3)]
    return worker, worker.fp.master.clone(), torch.tensor(losses, dtype=torch.float64)


@pytest.mark.parametrize("ckpt", [False, True])
def test_worker_matches_legacy(monkeypatch, ckpt):
    _, leg_a, loss_a = run_llama_tiny(monkeypatch, 7, ckpt)
    wl, leg_b, loss_b = run_llama_tiny(monkeypatch, 7, ckpt)
    wn, new, loss_n = run_llama_tiny(monkeypatch, 0, ckpt)
    assert not wl.fp.inplace_params
    assert not any(isinstance(m, WgradInplaceLinear) for m in wl.model.modules())
    # 2 blocks x (wq wk wv wo gate up down) + lm_head; embedding and norms are zeroed
    assert len(wn.fp.inplace_params) == 15
    assert sum(v.numel() for v in wn.fp._zero_views) == wn.fp.numel - sum(
        p.numel() for p in wn.fp.inplace_params)
    assert list(wn.model.state_dict()) == list(wl.model.state_dict())
    assert [p.shape for p in wn.fp.params] == [p.shape for p in wl.fp.params]
    assert_within_legacy_spread(f"llama-tiny ckpt={ckpt} master", new, leg_a, leg_b)
    assert torch.isfinite(loss_n).all()
    # the loss sums its rows with fp32 atomics in another order
    torch.testing.assert_close(loss_n, loss_a, rtol=1e-4, atol=0)


class TwiceAndNever(nn.Module):
    """One linear the forward never touches, one it calls twice, and a
    parameter that stays with autograd."""

    def __init__(self):
        super().__init__()
        self.never = nn.Linear(64, 64, bias=False)
        self.gain = nn.Parameter(torch.ones(64))
        self.twice = nn.Linear(64, 64, bias=False)

    def forward(self, x):
        h = self.twice(x) * self.gain
        return self.twice(h).float().pow(2).mean()


NEVER = slice(64, 64 + 64 * 64)  # never.weight in the flat buffers, behind gain


def run_twice_and_never(monkeypatch, ablate):
    monkeypatch.setenv("HYPHA_STEP_ABLATE", str(ablate))
    torch.manual_seed(3)
    model = TwiceAndNever()
    worker = DiLoCoWorker(model, DiLoCoConfig(h=100), comm=Comm(),
                          device=torch.device(DEV))
    # a module's own parameters come before its children's: gain, never, twice
    assert worker.fp.params[1] is model.never.weight
    never0 = worker.fp.master[NEVER].clone()
    if not ablate:
        assert len(worker.fp.inplace_params) == 2
        # what an earlier step would have left behind in a range nobody zeroes
        model.never.weight.grad.fill_(3.0)
    for step in range(2):
        x = rand_bf16(32, 64, seed=40 + step)
        model(x).backward()
        worker.inner_opt_step()
    return worker, worker.fp.master.clone(), never0


def test_stale_and_twice_used_gradients(monkeypatch):
    _, leg_a, _ = run_twice_and_never(monkeypatch, 7)
    _, leg_b, _ = run_twice_and_never(monkeypatch, 7)
    worker, new, never0 = run_twice_and_never(monkeypatch, 0)
    assert_within_legacy_spread("twice/never master", new, leg_a, leg_b)
    # the untouched weight: m = v = 0, so each step only decays it
    c = worker.cfg.inner
    want = never0.double()
    for step in range(2):
        want = want * (1.0 - lr_at(c, step) * c.weight_decay)
    torch.testing.assert_close(new[NEVER].double(), want, rtol=1e-6, atol=0)
    assert not (worker.model.never.weight.grad != 0).any()


def test_tied_weight_is_not_converted():
    """A weight two modules own keeps autograd's accumulation."""
    a = nn.Linear(16, 16, bias=False, device=DEV, dtype=torch.bfloat16)
    b = nn.Linear(16, 16, bias=False, device=DEV, dtype=torch.bfloat16)
    b.weight = a.weight
    biased = nn.Linear(16, 16, device=DEV, dtype=torch.bfloat16)
    lone = nn.Linear(16, 16, bias=False, device=DEV, dtype=torch.bfloat16)
    tree = nn.ModuleDict(dict(a=a, b=b, biased=biased, lone=lone))
    weights = convert_linears_to_wgrad_inplace(tree)
    assert len(weights) == 1 and weights[0] is lone.weight
    assert [type(m) for m in tree.values()] == [nn.Linear, nn.Linear, nn.Linear,
                                                WgradInplaceLinear]


# ---------------------------------------------------------------------------
# Shifted loss on unsliced logits
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("all_ignored", [False, True])
def test_shifted_loss_equals_sliced(all_ignored):
    b, s, v = 2, 5, 1024
    logits = rand_bf16(b, s, v, seed=50, scale=2.0)
    labels = torch.randint(0, v, (b, s), generator=gen(51)).to(DEV)
    labels[1, 2] = -100
    if all_ignored:
        labels.fill_(-100)
    la = logits.clone().requires_grad_()
    loss_a = ops.cross_entropy_loss(la, labels, shift=True)
    loss_a.backward()
    lb = logits.clone().requires_grad_()
    loss_b = ops.cross_entropy_loss(lb[:, :-1], labels[:, 1:])
    loss_b.backward()
    ga, gb = la.grad, lb.grad
    assert ga.shape == gb.shape == (b, s, v)
    ndiff = int((ga != gb).sum())
    print(f"all_ignored={all_ignored}: loss {loss_a.item():.6f} / {loss_b.item():.6f}, "
          f"{ndiff} gradient elements differ")
    assert ndiff == 0
    assert not (ga[:, -1] != 0).any(), "the last position has no target"
    assert not (ga[1, 1] != 0).any(), "position 1 of row 1 predicts an ignored label"
    if all_ignored:
        assert loss_a.item() == 0.0 and not (ga != 0).any()
    else:
        assert (ga[0, 0] != 0).any()
        # per-row terms are the same; their fp32 atomic sum runs in another order
        torch.testing.assert_close(loss_a, loss_b, rtol=1e-6, atol=0)
