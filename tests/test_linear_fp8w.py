"""Weight-only fp8 linears on the CPU: which modules quantize_linears_fp8_
swaps, Fp8Linear against F.linear on the dequantised weight, and the
infer-executor's "weight_quant" setting."""

import pytest
import torch
import torch.nn.functional as F

from hypha_amd import models
from hypha_amd.models import Fp8Linear, quantize_linears_fp8_
from hypha_amd.runtime.infer_executor import weight_quant


def swapped(model):
    return {n for n, m in model.named_modules() if isinstance(m, Fp8Linear)}


@pytest.mark.parametrize("tied", [False, True])
def test_quantize_swaps_the_expected_modules(tied):
    model = models.build("llama-tiny", tie_embeddings=tied).train()
    want = {f"blocks.{i}.{n}" for i in range(model.cfg.n_layers)
            for n in ("attn.wq", "attn.wk", "attn.wv", "attn.wo",
                      "mlp.w_gate", "mlp.w_up", "mlp.w_down")}
    if not tied:
        want.add("lm_head")
    embed = model.embed.weight
    assert quantize_linears_fp8_(model) is model and not model.training
    assert swapped(model) == want and model.embed.weight is embed
    assert not any(isinstance(m, torch.nn.Linear) for m in model.modules())
    before = dict(model.named_modules())
    quantize_linears_fp8_(model)  # idempotent: the same module objects
    assert dict(model.named_modules()) == before
    model.bfloat16()  # a cast changes no code and no scale
    assert model.lm_head is None or (model.lm_head.weight8.dtype == torch.float8_e4m3fn
                                     and model.lm_head.scale.dtype == torch.float32)


def test_other_linears_stay():
    model = torch.nn.Sequential(torch.nn.Linear(128, 64), torch.nn.Linear(192, 64, bias=False),
                                torch.nn.Linear(128, 40, bias=False))
    quantize_linears_fp8_(model)
    assert swapped(model) == set()


def test_fp8_linear_matches_dequantised_linear():
    torch.manual_seed(0)
    lin = torch.nn.Linear(256, 96, bias=False)
    q = Fp8Linear.from_linear(lin)
    x = torch.randn(2, 5, 256)
    w = q.weight8.float() * q.scale[:, None]
    torch.testing.assert_close(q(x), F.linear(x, w), rtol=1e-5, atol=1e-5)
    # per-row amax / 448: the quantisation error of a normal row stays below 2^-4 relative
    assert ((w - lin.weight).abs() <= lin.weight.abs() / 16 + q.scale[:, None] * 2 ** -9).all()


def test_weight_quant_setting():
    assert weight_quant({}) is None and weight_quant({"weight_quant": "fp8"}) == "fp8"
    with pytest.raises(ValueError):
        weight_quant({"weight_quant": "int4"})
    model = models.build("llama-tiny")
    with pytest.raises(ValueError):
        model.generate(torch.zeros(1, 4, dtype=torch.long), max_new_tokens=1, weight_quant="int8")
    model.generate(torch.zeros(1, 4, dtype=torch.long), max_new_tokens=2, weight_quant="fp8")
    assert "lm_head" in swapped(model)
