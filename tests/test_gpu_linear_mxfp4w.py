"""ops.linear_mxfp4w (ops/hip/linear_mxfp4w.hip) on the GPU: the kernel against
fp64 on the same MXFP4 weights, every e2m1 code and a range of block scales
exactly, the dispatch, and a quantised llama-tiny through prefill, eager decode
and the graphed decoder.

Bounds: those of test_gpu_linear_fp8w.py. rtol = atol = 3e-2 is the project's
bar for a bf16 MFMA GEMM; the relative L2 error must also stay within
FACTOR = 2.0 of a yardstick on the same GPU (the library on the same
dequantised bf16 operands; for the model, the unquantised bf16 model against
fp64 of its own parameters). Figures are printed (pytest -s)."""

import pytest
import torch

import model_ref64 as R
from hypha_amd import models, ops
from hypha_amd.models.kv_cache import KVCache
from hypha_amd.ops import interface
from hypha_amd.runtime.graphed_decode import GraphedDecoder

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TOL = 3e-2
FACTOR = 2.0
# e2m1 by code, written out: sign << 3 | index
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]


def make_inputs(M, N, K):
    g = torch.Generator(device=DEV).manual_seed(M + 31 * N + K)
    x = torch.randn(M, K, generator=g, device=DEV).bfloat16()
    codes, scales = ops.quantize_mxfp4(torch.randn(N, K, generator=g, device=DEV) / K ** 0.5)
    return x, codes, scales


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
    from hypha_amd import _C

    calls = []
    real = _C.linear_mxfp4w
    monkeypatch.setattr(_C, "linear_mxfp4w", lambda *a: (calls.append(1), real(*a))[1])
    x, codes, scales = make_inputs(M, N, K)
    want = x.double() @ ops.dequantize_mxfp4(codes, scales, torch.float64).T
    got = ops.linear_mxfp4w(x, codes, scales)
    assert len(calls) == 1 and got.shape == (M, N) and got.dtype == torch.bfloat16
    yard = x @ ops.dequantize_mxfp4(codes, scales, torch.bfloat16).t()
    err, err_yard = R.rel_l2(got, want), R.rel_l2(yard, want)
    print(f"LINEAR_MXFP4W | M={M} N={N} K={K} | rel_l2 kernel {err:.3e} | library {err_yard:.3e}")
    torch.testing.assert_close(got.double(), want, rtol=TOL, atol=TOL)
    assert err <= FACTOR * err_yard
    assert torch.equal(ops.linear_mxfp4w(x, codes, scales), got)  # no float atomics


@pytest.mark.parametrize("i", range(20))
@torch.no_grad()
def test_every_code_and_scale_exactly(i):
    """Row n holds the 16 codes cycling along k from a start that moves with n;
    block b of row n has the scale 2^((3 n + 5 b) % 9 - 4). x is a 32-column
    identity window, so the output is the weights of that window: this pins
    nibble order, selector order, scale placement and the A/B k agreement."""
    N, K = 64, 640  # two chunks, the second a half line for one k-wave only
    n, k = torch.arange(N, device=DEV)[:, None], torch.arange(K, device=DEV)[None, :]
    code = (k + n) % 16
    codes = (code[:, 0::2] | code[:, 1::2] << 4).to(torch.uint8)
    exp = (3 * n + 5 * torch.arange(K // 32, device=DEV)[None, :]) % 9 - 4
    scales = (exp + 127).to(torch.uint8)
    w = torch.tensor(E2M1, device=DEV)[code] * (2.0 ** exp.float()).repeat_interleave(32, 1)
    window = slice(32 * i, 32 * i + 32)
    x = torch.zeros(32, K, device=DEV, dtype=torch.bfloat16)
    x[:, window] = torch.eye(32, device=DEV, dtype=torch.bfloat16)
    assert torch.equal(ops.linear_mxfp4w(x, codes, scales), w[:, window].T.bfloat16())


@pytest.mark.parametrize("case", ["K=192", "N=40", "M=max_rows+1", "force_ref"])
@torch.no_grad()
def test_dispatch_takes_the_reference(case, monkeypatch):
    from hypha_amd import _C

    def boom(*a):
        raise AssertionError("_C.linear_mxfp4w called")

    M, N, K = {"K=192": (4, 64, 192), "N=40": (4, 40, 128),
               "M=max_rows+1": (interface.LINEAR_MXFP4W_MAX_ROWS + 1, 64, 128),
               "force_ref": (4, 64, 128)}[case]
    x, codes, scales = make_inputs(M, N, K)
    want = ops.reference.linear_mxfp4w(x, codes, scales)
    monkeypatch.setattr(_C, "linear_mxfp4w", boom)
    if case == "force_ref":
        monkeypatch.setenv("HYPHA_FORCE_REF", "1")
    assert torch.equal(ops.linear_mxfp4w(x, codes, scales), want)


@pytest.mark.parametrize("bad", ["code dtype", "scale shape"])
def test_value_errors(bad):
    x, codes, scales = make_inputs(2, 64, 128)
    with pytest.raises(ValueError):
        if bad == "code dtype":
            ops.linear_mxfp4w(x, codes.to(torch.int8), scales)
        else:
            ops.linear_mxfp4w(x, codes, scales[:, :-1])


def tiny(quantised):
    torch.manual_seed(0)
    m = R.unit_gain_(models.build("llama-tiny"), 0).to(DEV).bfloat16().eval()
    for buf in m.buffers():  # the RoPE tables stay fp32
        if buf.dtype == torch.bfloat16:
            buf.data = buf.data.float()
    return models.quantize_linears_mxfp4_(m) if quantised else m


def params64(model):
    """R.params64, with each quantised weight dequantised in fp64."""
    P = R.params64(model)
    for name, mod in model.named_modules():
        if isinstance(mod, models.Mxfp4Linear):
            P[name + ".weight"] = ops.dequantize_mxfp4(mod.codes, mod.scales, torch.float64).cpu()
    return P


@torch.no_grad()
def cached_logits_error(model, ids, steps):
    """rel-L2 against llama64 of the last-position logits after a prefill
    through a KV cache and after each of `steps` greedy single-token steps."""
    cfg, P = model.cfg, params64(model)
    caches = [KVCache(ids.shape[0], ids.shape[1] + steps, cfg.n_kv_heads, cfg.head_dim, DEV,
                      dtype=torch.bfloat16) for _ in model.blocks]
    got, want, x_in, pos = [], [], ids, 0
    for _ in range(steps + 1):
        x = model.embed(x_in)
        for blk, cache in zip(model.blocks, caches):
            x = blk(x, model.rope_cos, model.rope_sin, cache=cache, pos=pos)
        got.append(model.lm_head(model.norm(x[:, -1:]))[:, 0])
        want.append(R.llama64(P, cfg, ids.cpu())[0][:, -1])
        pos += x_in.shape[1]
        x_in = got[-1].argmax(-1, keepdim=True)
        ids = torch.cat([ids, x_in], 1)
    return R.rel_l2(torch.stack(got), torch.stack(want))


@torch.no_grad()
def test_model_logits_vs_fp64():
    ids = R.make_batch(512, 2, 8, 1)[0].to(DEV)
    err = cached_logits_error(tiny(True), ids, 4)
    err_bf16 = cached_logits_error(tiny(False), ids, 4)
    print(f"LINEAR_MXFP4W | llama-tiny logits rel_l2 mxfp4 weights {err:.3e} | bf16 {err_bf16:.3e}")
    assert err <= FACTOR * err_bf16


@torch.no_grad()
def test_graphed_decoder_matches_generate(monkeypatch):
    from hypha_amd import _C

    calls = []
    real = _C.linear_mxfp4w
    monkeypatch.setattr(_C, "linear_mxfp4w", lambda *a: (calls.append(1), real(*a))[1])
    model = tiny(True)
    assert isinstance(model.lm_head, models.Mxfp4Linear)
    ids = R.make_batch(512, 2, 8, 2)[0].to(DEV)
    want = model.generate(ids, max_new_tokens=12)
    dec = GraphedDecoder(model, 2, 8, 12)
    assert torch.equal(dec.generate(ids, 12), want)
    assert dec.graph is not None
    assert torch.equal(dec.generate(ids, 12), want)  # every step a replay of the graph
    assert calls
