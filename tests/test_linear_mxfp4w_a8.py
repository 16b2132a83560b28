"""MXFP8 activations for MXFP4 linears on the CPU: the quantiser's rules on
hand-made blocks, and the option values that select the mode."""

import pytest
import torch

from hypha_amd import models, ops
from hypha_amd.runtime.infer_executor import weight_quant


def hand_made_blocks():
    """[6, 32] bf16 with the wanted scale byte and dequantised block of each row."""
    x = torch.zeros(6, 32)
    want = torch.zeros(6, 32)
    byte = [2, 0, 0, 0, 0, 2]              # row 0: a block of zeros
    x[1, 3], byte[1] = -480.0 * 2.0 ** 5, 127 + 5   # amax 480 2^j saturates to 448 2^j
    want[1, 3] = -448.0 * 2.0 ** 5
    x[2, 0], x[2, 1], x[2, 2] = 256.0, 17.0, 19.0   # ulp 2 at 16: both are ties
    want[2, 0], want[2, 1], want[2, 2], byte[2] = 256.0, 16.0, 20.0, 127
    vals = torch.tensor([0.0, 2.0 ** -9, 0.875, 1.0, 1.125, 15.0, 208.0, 448.0])
    x[3] = torch.cat([vals, -vals, vals, -vals]) * 2.0 ** -20   # exact e4m3 values, scaled
    want[3], byte[3] = x[3], 127 - 20
    x[4, 31], byte[4] = 2.0 ** 120, 127 + 112   # a large exponent
    want[4, 31] = x[4, 31]
    x[5, 7] = 2.0 ** -130                     # the lower clamp: e = -125, code 2^-5
    want[5, 7] = x[5, 7]
    return x.bfloat16(), torch.tensor(byte, dtype=torch.uint8), want


def test_quantiser_properties():
    x, byte, want = hand_made_blocks()
    codes, scales = ops.quantize_mxfp8(x)
    assert codes.dtype == torch.float8_e4m3fn and codes.shape == x.shape
    assert torch.equal(scales[:, 0], byte)
    assert torch.equal(codes[0].float(), torch.zeros(32))
    assert codes[1, 3].float() == -448.0
    back = ops.dequantize_mxfp8(codes, scales, torch.float32)
    assert torch.equal(back, want)
    g = torch.Generator().manual_seed(0)
    r = (torch.randn(64, 96, generator=g) * 10.0 ** torch.randint(-3, 4, (64, 1), generator=g))
    back = ops.dequantize_mxfp8(*ops.quantize_mxfp8(r.bfloat16()), torch.float32)
    assert torch.isfinite(back).all() and torch.equal(back.bfloat16().float(), back)
    with pytest.raises(ValueError):
        ops.quantize_mxfp8(torch.zeros(2, 48))


@pytest.mark.parametrize("name", ["llama-tiny", "moe-tiny"])
@torch.no_grad()
def test_weight_quant_mxfp4_a8_is_accepted(name):
    assert weight_quant({"weight_quant": "mxfp4_a8"}) == "mxfp4_a8"
    torch.manual_seed(0)
    model = models.build(name)
    out = model.generate(torch.randint(0, 512, (2, 8)), max_new_tokens=3, prefill_chunk=4,
                         weight_quant="mxfp4_a8")
    assert out.shape == (2, 11)
    lins = [m for m in model.modules() if isinstance(m, models.Mxfp4Linear)]
    assert lins and all(m.act_quant == "mxfp8" for m in lins)
    models.quantize_linears_mxfp4_(model)   # and off again, on the linears already there
    assert all(m.act_quant is None for m in lins)


def test_bad_act_quant_raises():
    codes, scales = ops.quantize_mxfp4(torch.randn(64, 128))
    x = torch.randn(2, 128)
    want = ops.reference.linear_mxfp4w_a8(x, codes, scales)
    assert torch.equal(ops.linear_mxfp4w(x, codes, scales, act_quant="mxfp8"), want)
    for bad in ("fp8", "mxfp4", True):
        with pytest.raises(ValueError):
            ops.linear_mxfp4w(x, codes, scales, act_quant=bad)
    with pytest.raises(ValueError):
        models.quantize_linears_mxfp4_(torch.nn.Linear(128, 64, bias=False), act_quant="int8")
