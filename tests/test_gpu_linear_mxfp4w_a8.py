"""ops.linear_mxfp4w(..., act_quant="mxfp8") on the GPU (quantize_mxfp8_kernel
and linear_mxfp4w_a8_kernel in ops/hip/linear_mxfp4w.hip). Bounds: those of
test_gpu_linear_mxfp4w.py (rtol = atol = 3e-2; rel-L2 within FACTOR = 2.0 of the
library on the same dequantised bf16 operands); for the model the yardstick is
the same model under HYPHA_FORCE_REF=1. Figures are printed (pytest -s)."""

import pytest
import torch

import model_ref64 as R
from hypha_amd import models, ops
from hypha_amd.ops import interface
from hypha_amd.runtime.graphed_decode import GraphedDecoder
from test_gpu_linear_mxfp4w import E2M1, cached_logits_error
from test_gpu_linear_mxfp4w import make_inputs as make_bf16_inputs
from test_linear_mxfp4w_a8 import hand_made_blocks

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TOL = 3e-2
FACTOR = 2.0
A8 = dict(act_quant="mxfp8")


def counted(monkeypatch, name):
    from hypha_amd import _C

    calls, real = [], getattr(_C, name)
    monkeypatch.setattr(_C, name, lambda *a: (calls.append(1), real(*a))[1])
    return calls


def forbid(monkeypatch, *names):
    from hypha_amd import _C

    for name in names:
        monkeypatch.setattr(_C, name, lambda *a: pytest.fail("native binding called"))


@pytest.mark.parametrize("M,K", [(1, 128), (5, 640), (40, 4096)])
@torch.no_grad()
def test_quantise_kernel_vs_reference(M, K, monkeypatch):
    calls = counted(monkeypatch, "quantize_mxfp8")
    g = torch.Generator(device=DEV).manual_seed(M + K)
    x = torch.randn(M, K, generator=g, device=DEV)
    x *= 10.0 ** torch.randint(-3, 4, (M, K // 32), generator=g, device=DEV).repeat_interleave(32, 1)
    x = x.bfloat16()
    hand = hand_made_blocks()[0].to(DEV)          # six blocks into the first row(s)
    x.view(-1, 32)[:min(6, M * K // 32)] = hand[:M * K // 32]
    codes, scales = ops.quantize_mxfp8(x)
    want_codes, want_scales = ops.reference.quantize_mxfp8(x)
    assert calls and codes.dtype == torch.float8_e4m3fn
    assert torch.equal(scales, want_scales)
    assert torch.equal(codes.float(), want_codes.float())


@pytest.mark.parametrize("M,N,K", [
    (1, 64, 128),        # a half line; one wave with work
    (5, 96, 640),        # ragged tokens, an absent second tile, a K % 256 == 128 tail
    (32, 64, 1024),      # a full token tile through both LDS buffers
    (40, 64, 512),       # a second, partial token tile
    (8, 1024, 4096),     # split-K with the reduce kernel
    (8, 4096, 14336),    # w_down's reduction length
])
@torch.no_grad()
def test_kernel_vs_fp64(M, N, K, monkeypatch):
    calls = counted(monkeypatch, "linear_mxfp4w_a8")
    forbid(monkeypatch, "linear_mxfp4w")
    x, codes, scales = make_bf16_inputs(M, N, K)
    xq = ops.dequantize_mxfp8(*ops.reference.quantize_mxfp8(x), torch.float64)
    want = xq @ ops.dequantize_mxfp4(codes, scales, torch.float64).T
    got = ops.linear_mxfp4w(x, codes, scales, **A8)
    assert len(calls) == 1 and got.shape == (M, N) and got.dtype == torch.bfloat16
    yard = xq.bfloat16() @ ops.dequantize_mxfp4(codes, scales, torch.bfloat16).t()
    err, err_yard = R.rel_l2(got, want), R.rel_l2(yard, want)
    print(f"LINEAR_MXFP4W_A8 | M={M} N={N} K={K} | rel_l2 kernel {err:.3e} | library {err_yard:.3e}")
    torch.testing.assert_close(got.double(), want, rtol=TOL, atol=TOL)
    assert err <= FACTOR * err_yard
    assert torch.equal(ops.linear_mxfp4w(x, codes, scales, **A8), got)  # no float atomics


@pytest.mark.parametrize("side", ["weights", "activations"])
@pytest.mark.parametrize("i", range(20))
@torch.no_grad()
def test_every_code_and_scale_exactly(i, side):
    """Window i is k in [32 i, 32 i + 32) of N, K = 64, 640 (two chunks, the
    second a half line for one k-wave only).
    weights: test_gpu_linear_mxfp4w's matrix against an x whose window holds the
    diagonal 2^((t + 3 i) % 7 - 3) (one non-zero per block is exact in MXFP8):
    the output is the window's weights times those powers.
    activations: row n of W holds the code of 1.0 once, at k = 32 i + n % 32;
    every block of x holds 32 distinct e4m3 values in a k-dependent order under
    a scale that varies with (t, block): the output is the selected x times the
    weight's scale."""
    N, K = 64, 640
    n, k = torch.arange(N, device=DEV)[:, None], torch.arange(K, device=DEV)[None, :]
    b = torch.arange(K // 32, device=DEV)[None, :]
    t = torch.arange(32, device=DEV)[:, None]
    exp = (3 * n + 5 * b) % 9 - 4
    scales = (exp + 127).to(torch.uint8)
    wscale = (2.0 ** exp.float()).repeat_interleave(32, 1)
    window = slice(32 * i, 32 * i + 32)
    if side == "weights":
        code = (k + n) % 16
        w = torch.tensor(E2M1, device=DEV)[code] * wscale
        diag = 2.0 ** ((t[:, 0] + 3 * i) % 7 - 3).float()
        x = torch.zeros(32, K, device=DEV)
        x[:, window] = torch.diag(diag)
        want = w[:, window].T * diag[:, None]
    else:
        code = torch.where(k == 32 * i + n % 32, 2, 0)           # 0x2 is 1.0
        # 32 distinct e4m3 magnitudes per block (three mantissa bits), 8 .. 112
        # and 256: the largest is a power of two, so the block's scale is 2^0
        # before the factor; the order inside a block moves with t and the block
        j = (k % 32 * 5 + 7 * t + 3 * (k // 32)) % 32
        mag = torch.where(j == 31, 256.0, (8 + j % 8) * 2.0 ** (j // 8).float())
        sign = 1 - 2 * ((k + t) % 3 == 0).float()
        x = sign * mag * 2.0 ** ((5 * t + 3 * (k // 32)) % 11 - 5).float()
        want = x[:, window][:, torch.arange(N, device=DEV) % 32] * wscale[:, 32 * i][None, :]
    codes = (code[:, 0::2] | code[:, 1::2] << 4).to(torch.uint8)
    got = ops.linear_mxfp4w(x.bfloat16(), codes, scales, **A8)
    assert torch.equal(got, want.bfloat16())


@pytest.mark.parametrize("case", ["K=192", "N=40", "M=max_rows+1", "force_ref", "act_quant=None"])
@torch.no_grad()
def test_dispatch(case, monkeypatch):
    M, N, K = {"K=192": (4, 64, 192), "N=40": (4, 40, 128),
               "M=max_rows+1": (interface.LINEAR_MXFP4W_MAX_ROWS + 1, 64, 128),
               "force_ref": (4, 64, 128), "act_quant=None": (4, 64, 128)}[case]
    x, codes, scales = make_bf16_inputs(M, N, K)
    if case == "act_quant=None":
        want = ops.linear_mxfp4w(x, codes, scales)
        forbid(monkeypatch, "linear_mxfp4w_a8", "quantize_mxfp8")
        assert torch.equal(ops.linear_mxfp4w(x, codes, scales, act_quant=None), want)
        return
    forbid(monkeypatch, "linear_mxfp4w_a8", "linear_mxfp4w")
    if case == "force_ref":
        monkeypatch.setenv("HYPHA_FORCE_REF", "1")
    want = ops.reference.linear_mxfp4w_a8(x, codes, scales)
    assert torch.equal(ops.linear_mxfp4w(x, codes, scales, **A8), want)


def tiny(act_quant):
    torch.manual_seed(0)
    m = R.unit_gain_(models.build("llama-tiny"), 0).to(DEV).bfloat16().eval()
    for buf in m.buffers():  # the RoPE tables stay fp32
        if buf.dtype == torch.bfloat16:
            buf.data = buf.data.float()
    return models.quantize_linears_mxfp4_(m, act_quant=act_quant)


@torch.no_grad()
def test_model_logits_vs_fp64(monkeypatch):
    """Measured on an MI355X: see profiles/linear_mxfp4w_a8.md, section 5."""
    ids = R.make_batch(512, 2, 8, 1)[0].to(DEV)
    err = cached_logits_error(tiny("mxfp8"), ids, 4)
    err_w = cached_logits_error(tiny(None), ids, 4)
    monkeypatch.setenv("HYPHA_FORCE_REF", "1")
    err_ref = cached_logits_error(tiny("mxfp8"), ids, 4)
    print(f"LINEAR_MXFP4W_A8 | llama-tiny logits rel_l2 vs fp64 of the dequantised weights | "
          f"kernel {err:.3e} | reference route {err_ref:.3e} | weight-only mxfp4 {err_w:.3e}")
    assert err <= FACTOR * err_ref


@torch.no_grad()
def test_graphed_decoder_matches_generate(monkeypatch):
    calls = counted(monkeypatch, "linear_mxfp4w_a8")
    model = tiny("mxfp8")
    assert model.lm_head.act_quant == "mxfp8"
    ids = R.make_batch(512, 2, 8, 2)[0].to(DEV)
    want = model.generate(ids, max_new_tokens=12)
    dec = GraphedDecoder(model, 2, 8, 12)
    assert torch.equal(dec.generate(ids, 12), want)
    assert dec.graph is not None
    assert torch.equal(dec.generate(ids, 12), want)  # every step a replay of the graph
    assert calls
