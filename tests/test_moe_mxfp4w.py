"""Weight-only MXFP4 experts on the CPU: MoEMLP.quantize_experts_mxfp4_, its
refusals, reference.moe_ffn_mxfp4w against reference.moe_ffn on the
dequantised weights, and the quantised forward against an unquantised copy."""

import copy

import pytest
import torch

from hypha_amd import ops
from hypha_amd.models.moe import PRESETS, MoEMLP

CFG = PRESETS["moe-tiny"]
E, H, F = CFG.n_experts, CFG.hidden_size, CFG.ffn_hidden


def test_quantize_is_idempotent_and_survives_a_cast():
    mlp = MoEMLP(CFG).train()
    assert not mlp.experts_mxfp4
    assert mlp.quantize_experts_mxfp4_() is mlp and mlp.experts_mxfp4 and not mlp.training
    assert [n for n, _ in mlp.named_parameters()] == ["router.weight"]
    before = {n: b.clone() for n, b in mlp.named_buffers()}
    assert {n: tuple(b.shape) for n, b in before.items()} == {
        "c_gate": (E, F, H // 2), "e_gate": (E, F, H // 32), "c_up": (E, F, H // 2),
        "e_up": (E, F, H // 32), "c_down": (E, H, F // 2), "e_down": (E, H, F // 32)}
    mlp.quantize_experts_mxfp4_().bfloat16()
    assert mlp.router.weight.dtype == torch.bfloat16
    for n, b in mlp.named_buffers():
        assert b.dtype == torch.uint8 and torch.equal(b, before[n])
    with pytest.raises(RuntimeError):  # inference only: grad is enabled here
        mlp(torch.zeros(1, 2, H, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError), torch.no_grad():
        mlp.train()(torch.zeros(1, 2, H, dtype=torch.bfloat16))


def test_refusals():
    sharded = MoEMLP(CFG)
    sharded.ep = (0, 2, None)
    with pytest.raises(ValueError):
        sharded.quantize_experts_mxfp4_()
    with pytest.raises(ValueError):
        MoEMLP(CFG).quantize_experts_fp8_().quantize_experts_mxfp4_()
    with pytest.raises(ValueError):
        MoEMLP(CFG).quantize_experts_mxfp4_().quantize_experts_fp8_()


@torch.no_grad()
def test_reference_is_moe_ffn_on_the_dequantised_weights():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(9, H, generator=g).bfloat16()
    logits = torch.randn(9, E, generator=g)
    ws = [torch.randn(E, r, c, generator=g) / c ** 0.5 for r, c in ((F, H), (F, H), (H, F))]
    quant = [t for w in ws for t in ops.quantize_mxfp4(w)]
    deq = [ops.dequantize_mxfp4(quant[2 * i], quant[2 * i + 1]) for i in range(3)]
    want = ops.reference.moe_ffn(x, logits, *deq, CFG.top_k)
    assert torch.equal(ops.reference.moe_ffn_mxfp4w(x, logits, *quant, CFG.top_k), want)
    assert torch.equal(ops.moe_ffn_mxfp4w(x, logits, *quant, CFG.top_k), want)  # CPU: reference


@torch.no_grad()
def test_forward_matches_the_dequantised_module():
    torch.manual_seed(1)
    plain = MoEMLP(CFG).eval()
    for w in (plain.w_gate, plain.w_up, plain.w_down):
        torch.nn.init.normal_(w, std=w.shape[-1] ** -0.5)
    quant = copy.deepcopy(plain).quantize_experts_mxfp4_()
    for n in ("gate", "up", "down"):
        getattr(plain, "w_" + n).copy_(ops.dequantize_mxfp4(
            getattr(quant, "c_" + n), getattr(quant, "e_" + n), torch.float32))
    x = torch.randn(2, 9, H)
    torch.testing.assert_close(quant(x)[0], plain(x)[0], rtol=1e-5, atol=1e-5)
