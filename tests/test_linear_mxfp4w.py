"""Weight-only MXFP4 on the CPU: the format (ops.quantize_mxfp4 and
ops.dequantize_mxfp4), which modules quantize_linears_mxfp4_ swaps, and the
"weight_quant" setting."""

import pytest
import torch

from hypha_amd import models, ops
from hypha_amd.models import Fp8Linear, Mxfp4Linear, quantize_linears_fp8_, quantize_linears_mxfp4_
from hypha_amd.runtime.infer_executor import weight_quant

# e2m1 by code, written out: sign << 3 | index
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]


def test_dequantize_matches_the_table():
    code = torch.arange(64) % 16  # element k of each row; element 2 i is byte i's low nibble
    codes = (code[0::2] | code[1::2] << 4).to(torch.uint8).expand(3, 32).contiguous()
    scales = torch.tensor([[2, 127], [130, 124], [252, 1 + 127]], dtype=torch.uint8)
    want = torch.tensor(E2M1, dtype=torch.float64)[code] * torch.pow(
        2.0, scales.double() - 127).repeat_interleave(32, 1)
    assert torch.equal(ops.dequantize_mxfp4(codes, scales, torch.float64), want)
    assert torch.equal(ops.dequantize_mxfp4(codes, scales).double(), want)  # bf16 holds them all


def test_round_trip_and_zero_block():
    g = torch.Generator().manual_seed(0)
    nib = torch.randint(0, 16, (64, 256), generator=g)
    nib[nib == 8] = 0  # zero is always 0x0
    nib[:, 7::32] = 7  # every block reaches magnitude 6, so its scale is recovered
    nib[5, 32:64] = 0  # an all-zero block takes the lower clamp
    codes = (nib[:, 0::2] | nib[:, 1::2] << 4).to(torch.uint8)
    scales = torch.randint(2, 253, (64, 8), generator=g).to(torch.uint8)
    scales[5, 1] = 2
    w = ops.dequantize_mxfp4(codes, scales, torch.float32)
    assert (w[5, 32:64] == 0).all() and torch.isfinite(w).all()
    codes2, scales2 = ops.quantize_mxfp4(w)
    assert torch.equal(codes2, codes) and torch.equal(scales2, scales)
    # the rule on plain weights: scale from amax, saturation at 6, ties to the even code
    t = torch.zeros(1, 32)
    t[0, :9] = torch.tensor([7.9, 5.0, 3.5, 2.5, 1.75, 1.25, 0.75, -0.25, -5.1])
    c, s = ops.quantize_mxfp4(t)
    assert s.item() == 127 and ops.dequantize_mxfp4(c, s, torch.float32)[0, :9].tolist() == [
        6.0, 4.0, 4.0, 2.0, 2.0, 1.0, 1.0, 0.0, -6.0]
    assert c[0, 3].item() == 0x02  # high nibble: -0.25 rounds to 0x0, not to negative zero


@pytest.mark.parametrize("tied", [False, True])
def test_quantize_swaps_what_the_fp8_pass_swaps(tied):
    def swapped(model, cls):
        return {n for n, m in model.named_modules() if isinstance(m, cls)}

    model = models.build("llama-tiny", tie_embeddings=tied).train()
    want = swapped(quantize_linears_fp8_(models.build("llama-tiny", tie_embeddings=tied)),
                   Fp8Linear)
    embed = model.embed.weight
    assert quantize_linears_mxfp4_(model) is model and not model.training
    assert swapped(model, Mxfp4Linear) == want and ("lm_head" in want) != tied
    assert model.embed.weight is embed
    model.bfloat16()  # a cast changes no code and no scale
    assert all(b.dtype == torch.uint8 for m in model.modules() if isinstance(m, Mxfp4Linear)
               for b in m.buffers())


def test_weight_quant_setting():
    assert weight_quant({"weight_quant": "mxfp4"}) == "mxfp4"
    with pytest.raises(ValueError):
        weight_quant({"weight_quant": "int4"})
    model = models.build("llama-tiny")
    ids = torch.zeros(1, 4, dtype=torch.long)
    assert model.generate(ids, max_new_tokens=2, weight_quant="mxfp4").shape == (1, 6)
    assert isinstance(model.lm_head, Mxfp4Linear)
    moe = models.build("moe-tiny")
    assert moe.generate(ids, max_new_tokens=2, weight_quant="mxfp4").shape == (1, 6)
