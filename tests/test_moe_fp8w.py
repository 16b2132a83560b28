"""Weight-only fp8 experts on the CPU: MoEMLP.quantize_experts_fp8_, the
quantised forward against an unquantised copy on the dequantised weights,
what quantize_linears_fp8_ does to the MoE family, and generate's keyword."""

import copy

import pytest
import torch

from hypha_amd import models
from hypha_amd.models import quantize_linears_fp8_
from hypha_amd.models.moe import PRESETS, MoEMLP


def test_quantize_is_idempotent_and_survives_a_cast():
    mlp = MoEMLP(PRESETS["moe-tiny"]).train()
    assert mlp.quantize_experts_fp8_() is mlp and not mlp.training
    assert [n for n, _ in mlp.named_parameters()] == ["router.weight"]
    before = {n: b.clone() for n, b in mlp.named_buffers()}
    mlp.quantize_experts_fp8_().bfloat16()
    assert mlp.router.weight.dtype == torch.bfloat16 and len(before) == 6
    for n, b in mlp.named_buffers():
        assert b.dtype == before[n].dtype
        assert torch.equal(b.view(torch.uint8), before[n].view(torch.uint8))
    with pytest.raises(RuntimeError):  # inference only: grad is enabled here
        mlp(torch.zeros(1, 2, 128, dtype=torch.bfloat16))
    sharded = MoEMLP(PRESETS["moe-tiny"])
    sharded.ep = (0, 2, None)
    with pytest.raises(ValueError):
        sharded.quantize_experts_fp8_()


@torch.no_grad()
def test_forward_matches_the_dequantised_module():
    torch.manual_seed(1)
    cfg = PRESETS["moe-tiny"]
    plain = MoEMLP(cfg).eval()
    for w in (plain.w_gate, plain.w_up, plain.w_down):
        torch.nn.init.normal_(w, std=w.shape[-1] ** -0.5)
    quant = copy.deepcopy(plain).quantize_experts_fp8_()
    for n in ("gate", "up", "down"):
        codes, scale = getattr(quant, f"w_{n}8"), getattr(quant, f"s_{n}")
        getattr(plain, "w_" + n).copy_(codes.float() * scale[..., None])
    x = torch.randn(2, 9, cfg.hidden_size)
    torch.testing.assert_close(quant(x)[0], plain(x)[0], rtol=1e-5, atol=1e-5)


def test_quantize_linears_and_generate_cover_the_moe_family():
    model = quantize_linears_fp8_(models.build("moe-tiny"))
    mlps = [m for m in model.modules() if isinstance(m, MoEMLP)]
    assert len(mlps) == model.cfg.n_layers and all(m.experts_fp8 for m in mlps)
    assert all(type(m.router) is torch.nn.Linear for m in mlps)
    model = models.build("moe-tiny")
    ids = torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(ValueError):
        model.generate(ids, max_new_tokens=1, weight_quant="int8")
    assert model.generate(ids, max_new_tokens=2, weight_quant="fp8").shape == (1, 6)
    assert not any(p.dim() == 3 for p in model.parameters())
