"""MXFP8 activations inside the MXFP4 expert FFN on the CPU: the op against
reference.moe_ffn_mxfp4w_a8, its refusals, and the option value that selects
the mode for a model."""

import pytest
import torch

from hypha_amd import models, ops
from hypha_amd.models.moe import PRESETS, MoEMLP
from hypha_amd.runtime.infer_executor import weight_quant

CFG = PRESETS["moe-tiny"]
E, H, F = CFG.n_experts, CFG.hidden_size, CFG.ffn_hidden


def make_inputs():
    g = torch.Generator().manual_seed(4)
    ws = [torch.randn(E, r, c, generator=g) / c ** 0.5 for r, c in ((F, H), (F, H), (H, F))]
    quant = [t for w in ws for t in ops.quantize_mxfp4(w)]
    return (torch.randn(9, H, generator=g).bfloat16(), torch.randn(9, E, generator=g), *quant)


@torch.no_grad()
def test_op_is_the_reference_and_another_mode():
    args = make_inputs()
    want = ops.reference.moe_ffn_mxfp4w_a8(*args, CFG.top_k)
    got = ops.moe_ffn_mxfp4w(*args, CFG.top_k, act_quant="mxfp8")
    assert got.dtype == torch.bfloat16 and torch.equal(got, want)
    plain = ops.moe_ffn_mxfp4w(*args, CFG.top_k)
    assert torch.equal(plain, ops.moe_ffn_mxfp4w(*args, CFG.top_k, act_quant=None))
    assert not torch.equal(got, plain)
    torch.testing.assert_close(got.float(), plain.float(), rtol=0.1, atol=0.1)


def test_bad_act_quant_raises():
    args = make_inputs()
    for bad in ("fp8", "mxfp4", True):
        with pytest.raises(ValueError):
            ops.moe_ffn_mxfp4w(*args, CFG.top_k, act_quant=bad)
    with pytest.raises(ValueError):
        MoEMLP(CFG).quantize_experts_mxfp4_(act_quant="int8")
    with pytest.raises(ValueError):
        models.quantize_linears_mxfp4_(MoEMLP(CFG), expert_act_quant="int8")


@torch.no_grad()
def test_weight_quant_mxfp4_experts_a8():
    assert weight_quant({"weight_quant": "mxfp4_experts_a8"}) == "mxfp4_experts_a8"
    torch.manual_seed(0)
    model = models.build("moe-tiny")
    out = model.generate(torch.randint(0, 512, (2, 8)), max_new_tokens=3, prefill_chunk=4,
                         weight_quant="mxfp4_experts_a8")
    assert out.shape == (2, 11)
    mlps = [m for m in model.modules() if isinstance(m, MoEMLP)]
    lins = [m for m in model.modules() if isinstance(m, models.Mxfp4Linear)]
    assert mlps and all(m.experts_mxfp4 and m.act_quant == "mxfp8" for m in mlps)
    assert lins and all(m.act_quant is None for m in lins)
    models.quantize_linears_mxfp4_(model)  # and off again, on the experts already quantised
    assert all(m.act_quant is None for m in mlps)
