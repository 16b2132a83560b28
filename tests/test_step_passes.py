"""CPU side of the training-step changes: shift=True and grad_scale mean on
the reference path exactly what the callers used to spell out, and a CPU
worker keeps autograd's weight gradients and a whole-buffer zero_grad."""

import torch
import torch.nn as nn

from hypha_amd import models, ops
from hypha_amd.parallel import Comm, DiLoCoConfig, DiLoCoWorker
from hypha_amd.parallel.diloco import WgradInplaceLinear


def test_shifted_loss_is_the_sliced_loss():
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(2, 5, 37, generator=g)
    labels = torch.randint(0, 37, (2, 5), generator=g)
    labels[1, 2] = -100
    a = logits.clone().requires_grad_()
    b = logits.clone().requires_grad_()
    la = ops.cross_entropy_loss(a, labels, shift=True)
    lb = ops.cross_entropy_loss(b[:, :-1], labels[:, 1:])
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)
    assert not (a.grad[:, -1] != 0).any()
    for bad in (logits[0], logits[:, :4]):
        try:
            ops.cross_entropy_loss(bad, labels, shift=True)
        except ValueError:
            continue
        raise AssertionError("shift=True must refuse operands that are not [B, S, V] / [B, S]")


def test_fused_adamw_grad_scale_reference():
    g = torch.Generator().manual_seed(1)
    n = 1000
    hp = dict(lr=1e-2, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.1, step=1)
    grad = torch.randn(n, generator=g)
    coef = torch.tensor(0.3)

    def state():
        master = torch.randn(n, generator=torch.Generator().manual_seed(2))
        return [master, master.clone(), torch.zeros(n), torch.zeros(n)]

    new, old = state(), state()
    kept = grad.clone()
    ops.fused_adamw(new[0], new[1], grad, new[2], new[3], grad_scale=coef, **hp)
    assert torch.equal(grad, kept)
    ops.fused_adamw(old[0], old[1], grad.clone().mul_(coef), old[2], old[3], **hp)
    for a, b in zip(new, old):
        assert torch.equal(a, b)


def test_cpu_worker_keeps_autograd_wgrad():
    torch.manual_seed(0)
    worker = DiLoCoWorker(models.build("llama-tiny"), DiLoCoConfig(h=100), comm=Comm(),
                          device=torch.device("cpu"))
    assert not worker.fp.inplace_params
    assert not any(isinstance(m, WgradInplaceLinear) for m in worker.model.modules())
    worker.fp.flat_grad.fill_(1.0)
    worker.fp.zero_grad()
    assert not worker.fp.flat_grad.any()


def test_wgrad_inplace_linear_on_cpu_is_a_linear():
    lin = nn.Linear(8, 4, bias=False)
    mod = WgradInplaceLinear.from_linear(lin)
    assert mod.weight is lin.weight and isinstance(mod, nn.Linear) and mod.bias is None
    assert list(mod.state_dict()) == ["weight"]
    x = torch.randn(3, 8, requires_grad=True)
    mod(x).sum().backward()
    xr = x.detach().clone().requires_grad_()
    ref = nn.Linear(8, 4, bias=False)
    ref.weight.data.copy_(lin.weight.data)
    ref(xr).sum().backward()
    assert torch.equal(x.grad, xr.grad) and torch.equal(mod.weight.grad, ref.weight.grad)
