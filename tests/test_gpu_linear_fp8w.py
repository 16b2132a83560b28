"""ops.linear_fp8w (ops/hip/linear_fp8w.hip) on the GPU: the kernel against
fp64 on the same e4m3 weights, every e4m3 code exactly, the dispatch, and a
quantised llama-tiny through prefill, eager decode and the graphed decoder.

Bounds: rtol = atol = 3e-2 is the project's bar for a bf16 MFMA GEMM; the
relative L2 error must also stay within FACTOR = 2.0 of a yardstick on the
same GPU (the library on the same operands; for the model, the unquantised
bf16 model against fp64 of its own parameters). Figures are printed
(pytest -s)."""

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


def make_inputs(M, N, K):
    g = torch.Generator(device=DEV).manual_seed(M + 31 * N + K)
    x = torch.randn(M, K, generator=g, device=DEV).bfloat16()
    w8, scale = ops.quantize_rows_e4m3(torch.randn(N, K, generator=g, device=DEV) / K ** 0.5)
    return x, w8, scale


@pytest.mark.parametrize("M,N,K", [
    (1, 64, 128),        # one chunk, one wave with work
    (5, 96, 640),        # ragged tokens, second tile of the last workgroup past N, a chunk tail
    (32, 64, 1024),      # a full token tile, two chunks through both LDS buffers
    (40, 64, 512),       # a second, partial token tile
    (8, 1024, 4096),     # split-K with the reduce kernel, Llama's wk
    (8, 4096, 14336),    # w_down's reduction length
])
@torch.no_grad()
def test_kernel_vs_fp64(M, N, K, monkeypatch):
    from hypha_amd import _C

    calls = []
    real = _C.linear_fp8w
    monkeypatch.setattr(_C, "linear_fp8w", lambda *a: (calls.append(1), real(*a))[1])
    x, w8, scale = make_inputs(M, N, K)
    want = x.double() @ (w8.float().double() * scale.double()[:, None]).T
    got = ops.linear_fp8w(x, w8, scale)
    assert len(calls) == 1 and got.shape == (M, N) and got.dtype == torch.bfloat16
    yard = ((x @ w8.bfloat16().t()).float() * scale).bfloat16()
    err, err_yard = R.rel_l2(got, want), R.rel_l2(yard, want)
    print(f"LINEAR_FP8W | M={M} N={N} K={K} | rel_l2 kernel {err:.3e} | library {err_yard:.3e}")
    torch.testing.assert_close(got.double(), want, rtol=TOL, atol=TOL)
    assert err <= FACTOR * err_yard
    assert torch.equal(ops.linear_fp8w(x, w8, scale), got)  # no float atomics


@pytest.mark.parametrize("i", range(8))
@torch.no_grad()
def test_every_code_exactly(i):
    N, K = 64, 256
    codes = torch.arange(K, dtype=torch.uint8, device=DEV)
    codes[codes & 0x7f == 0x7f] = 0  # the two NaN codes
    w8 = codes.view(torch.float8_e4m3fn).expand(N, K).contiguous()
    scale = 2.0 ** (torch.arange(N, device=DEV) % 5 - 2).float()
    window = slice(32 * i, 32 * i + 32)
    x = torch.zeros(32, K, device=DEV, dtype=torch.bfloat16)
    x[:, window] = torch.eye(32, device=DEV, dtype=torch.bfloat16)
    want = (w8.float()[:, window].T * scale).bfloat16()
    assert torch.equal(ops.linear_fp8w(x, w8, scale), want)


@pytest.mark.parametrize("case", ["K=192", "N=40", "M=max_rows+1", "force_ref"])
@torch.no_grad()
def test_dispatch_takes_the_reference(case, monkeypatch):
    from hypha_amd import _C

    def boom(*a):
        raise AssertionError("_C.linear_fp8w called")

    M, N, K = {"K=192": (4, 64, 192), "N=40": (4, 40, 128),
               "M=max_rows+1": (interface.LINEAR_FP8W_MAX_ROWS + 1, 64, 128),
               "force_ref": (4, 64, 128)}[case]
    x, w8, scale = make_inputs(M, N, K)
    want = ops.reference.linear_fp8w(x, w8, scale)
    monkeypatch.setattr(_C, "linear_fp8w", boom)
    if case == "force_ref":
        monkeypatch.setenv("HYPHA_FORCE_REF", "1")
    assert torch.equal(ops.linear_fp8w(x, w8, scale), want)


@pytest.mark.parametrize("bad", ["w8 dtype", "scale length"])
def test_value_errors(bad):
    x, w8, scale = make_inputs(2, 64, 128)
    with pytest.raises(ValueError):
        if bad == "w8 dtype":
            ops.linear_fp8w(x, w8.bfloat16(), scale)
        else:
            ops.linear_fp8w(x, w8, scale[:-1])


def tiny(quantised):
    torch.manual_seed(0)
    m = R.unit_gain_(models.build("llama-tiny"), 0).to(DEV).bfloat16().eval()
    for buf in m.buffers():  # the RoPE tables stay fp32
        if buf.dtype == torch.bfloat16:
            buf.data = buf.data.float()
    return models.quantize_linears_fp8_(m) if quantised else m


def params64(model):
    """R.params64, with each quantised weight as weight8 * scale in fp64."""
    P = R.params64(model)
    for name, mod in model.named_modules():
        if isinstance(mod, models.Fp8Linear):
            P[name + ".weight"] = (mod.weight8.double() * mod.scale.double()[:, None]).cpu()
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
    print(f"LINEAR_FP8W | llama-tiny logits rel_l2 fp8 weights {err:.3e} | bf16 {err_bf16:.3e}")
    assert err <= FACTOR * err_bf16


@pytest.mark.parametrize("quantised", [True, False])
@torch.no_grad()
def test_graphed_decoder_matches_generate(quantised, monkeypatch):
    from hypha_amd import _C

    calls = []
    real = _C.linear_fp8w
    monkeypatch.setattr(_C, "linear_fp8w", lambda *a: (calls.append(1), real(*a))[1])
    model = tiny(quantised)
    assert isinstance(model.lm_head, models.Fp8Linear) == quantised
    ids = R.make_batch(512, 2, 8, 2)[0].to(DEV)
    want = model.generate(ids, max_new_tokens=12)
    dec = GraphedDecoder(model, 2, 8, 12)
    assert torch.equal(dec.generate(ids, 12), want)
    assert dec.graph is not None
    assert torch.equal(dec.generate(ids, 12), want)  # every step a replay of the graph
    assert bool(calls) == quantised
