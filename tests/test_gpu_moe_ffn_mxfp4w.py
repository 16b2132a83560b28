"""ops.moe_ffn_mxfp4w (moe_expert_mxfp4w_kernel in ops/hip/moe_ffn.hip) on the
GPU against an fp64 reference written here, its dispatch, a quantised MoEMLP
and a model. Block b (32 k) of row r of expert e of matrix m (gate, up, down =
0, 1, 2) is scaled by 2 ** ((b + r + 3 e + m) % 5 - 3) before quantisation, so
a scale byte read at the wrong block, row, expert or matrix is up to 16x off.
Bounds: rtol = atol = 3e-2, the bar for a bf16 MFMA GEMM chain, and a relative
L2 error within FACTOR = 2.0 of reference.moe_ffn_mxfp4w's (the library on the
same operands); both are printed (profiles/moe_ffn_mxfp4w.md, section 5)."""

import pytest
import torch
import torch.nn as nn

from hypha_amd import models, ops
from hypha_amd.models.moe import MoEMLP

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TOL = 3e-2
FACTOR = 2.0


def make_inputs(T, E, K, h, f, routing, seed=0):
    """-> x ~ N(0, 1), logits, (codes, scales) of N(0, 1/fan_in) x block factors"""
    g = torch.Generator(device=DEV).manual_seed(seed + 7919 * T + h)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    ar = lambda n: torch.arange(n, device=DEV)
    x = rn(T, h).bfloat16()
    quant = []
    for m, (rows, cols) in enumerate(((f, h), (f, h), (h, f))):
        p = ar(cols // 32)[None, None, :] + ar(rows)[None, :, None] + 3 * ar(E)[:, None, None] + m
        w = rn(E, rows, cols // 32, 32) / cols ** 0.5 * (2.0 ** (p % 5 - 3))[..., None]
        quant += ops.quantize_mxfp4(w.reshape(E, rows, cols).bfloat16())
    logits = rn(T, E)
    if routing == "expert2":
        logits[:, 2] += 30.0
    return (x, logits, *quant)


def ref64(x, logits, cg, eg, cu, eu, cd, ed, K):
    """fp64, lowest index wins ties, one expert's dequantised weights at a
    time. -> (out, topi, topw)"""
    probs = torch.softmax(logits.double(), -1)
    topi = torch.sort(probs, dim=-1, descending=True, stable=True).indices[:, :K]
    topw = probs.gather(1, topi)
    topw = topw / topw.sum(-1, keepdim=True)
    out = torch.zeros(x.shape, dtype=torch.float64, device=x.device)
    for e in range(cg.shape[0]):
        g64, u64, d64 = (ops.dequantize_mxfp4(c[e], s[e], torch.float64)
                         for c, s in ((cg, eg), (cu, eu), (cd, ed)))
        for t, k in (topi == e).nonzero().tolist():
            xt = x[t].double()
            g = g64 @ xt
            out[t] += topw[t, k] * (d64 @ (g / (1 + torch.exp(-g)) * (u64 @ xt)))
    return out, topi, topw


rel_l2 = lambda a, b: ((a.double() - b).norm() / b.norm()).item()


# the kernel's chunk is 512 k, a wave's line 256 k, so the shapes need no shift
@pytest.mark.parametrize("T,E,K,h,f,routing", [
    (1, 4, 2, 128, 256, "random"),       # early exit; h = half a line: one k-wave has no k
    (5, 4, 2, 640, 384, "random"),       # ragged counts; a half-line tail in both stages
    (40, 4, 1, 128, 256, "expert2"),     # 40 > 32: a second, partial token tile
    (33, 8, 2, 2176, 1664, "random"),    # 5 chunks > depth + LDS buffers, half-line end; split-K
    (8, 2, 2, 4096, 14336, "random"),    # Mixtral's reduction lengths
])
@torch.no_grad()
def test_ffn_vs_fp64(T, E, K, h, f, routing):
    args = make_inputs(T, E, K, h, f, routing)
    want, topi, topw = ref64(*args, K)
    if routing == "expert2":
        assert (topi == 2).all()
    got = ops.moe_ffn_mxfp4w(*args, K)
    assert got.shape == args[0].shape and got.dtype == torch.bfloat16
    assert torch.isfinite(got).all()
    err = rel_l2(got, want)
    err_loop = rel_l2(ops.reference.moe_ffn_mxfp4w(*args, K), want)
    print(f"MOE_FFN_MXFP4W | T={T} E={E} K={K} h={h} f={f} | rel_l2 fused {err:.3e} | "
          f"library loop {err_loop:.3e} | max abs {(got.double() - want).abs().max():.3e}")
    torch.testing.assert_close(got.double(), want, rtol=TOL, atol=TOL)
    assert err <= FACTOR * err_loop
    assert torch.equal(ops.moe_ffn_mxfp4w(*args, K), got)  # no float atomics


def counted(monkeypatch):
    from hypha_amd import _C

    calls, real = [], _C.moe_ffn_mxfp4w
    monkeypatch.setattr(_C, "moe_ffn_mxfp4w",
                        lambda *a: (calls.append(a[0].shape[0]), real(*a))[1])
    return calls


@pytest.mark.parametrize("why", ["odd_width", "force_ref"])
@torch.no_grad()
def test_takes_the_reference(why, monkeypatch):
    from hypha_amd import _C

    args = make_inputs(5, 4, 2, 128, 192 if why == "odd_width" else 256, "random")
    if why == "force_ref":
        monkeypatch.setenv("HYPHA_FORCE_REF", "1")
    want = ops.reference.moe_ffn_mxfp4w(*args, 2)
    monkeypatch.setattr(_C, "moe_ffn_mxfp4w", lambda *a: pytest.fail("_C.moe_ffn_mxfp4w called"))
    assert torch.equal(ops.moe_ffn_mxfp4w(*args, 2), want)


def test_value_errors():
    x, logits, cg, eg, cu, eu, cd, ed = make_inputs(2, 4, 2, 128, 128, "random")
    with pytest.raises(ValueError):
        ops.moe_ffn_mxfp4w(x, logits, cg.bfloat16(), eg, cu, eu, cd, ed, 2)
    with pytest.raises(ValueError):
        ops.moe_ffn_mxfp4w(x, logits, cg, eg[..., :-1], cu, eu, cd, ed, 2)


@pytest.fixture
def tiny_mlp():
    torch.manual_seed(3)
    cfg = models.moe.PRESETS["moe-tiny"]
    mlp = MoEMLP(cfg)
    for w in (mlp.router.weight, mlp.w_gate, mlp.w_up):  # O(1) activations
        nn.init.normal_(w, std=cfg.hidden_size ** -0.5)
    nn.init.normal_(mlp.w_down, std=cfg.ffn_hidden ** -0.5)
    return mlp.to(DEV).bfloat16().quantize_experts_mxfp4_()


def mlp_ref64(mlp, xf):
    return ref64(xf, mlp.router(xf).float(), mlp.c_gate, mlp.e_gate, mlp.c_up, mlp.e_up,
                 mlp.c_down, mlp.e_down, mlp.cfg.top_k)


@torch.no_grad()
def test_module_dispatch(tiny_mlp, monkeypatch):
    calls = counted(monkeypatch)
    x = torch.randn(1, 4, tiny_mlp.cfg.hidden_size, device=DEV).bfloat16()
    fused, _ = tiny_mlp(x)
    assert calls == [4]
    monkeypatch.setattr(tiny_mlp.cfg, "fused_ffn_mxfp4_max_tokens", 0)
    loop, _ = tiny_mlp(x)
    assert calls == [4]
    want = mlp_ref64(tiny_mlp, x[0])[0]
    for got in (fused, loop):
        torch.testing.assert_close(got[0].double(), want, rtol=TOL, atol=TOL)


@torch.no_grad()
def test_captured_mlp_replays_under_new_routing(tiny_mlp):
    mlp = tiny_mlp
    cand = torch.randn(16, 1, 1, mlp.cfg.hidden_size, device=DEV).bfloat16()  # [cand, b, s, h]
    sets = [set(mlp_ref64(mlp, c[0])[1].reshape(-1).tolist()) for c in cand]
    second = next((i for i in range(1, 16) if sets[i] - sets[0]), None)
    assert second is not None  # an expert with no token at capture gets one at replay
    x_static = cand[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mlp(x_static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_static, _ = mlp(x_static)
    for i in (second, 0):
        x_static.copy_(cand[i])
        graph.replay()
        want = mlp_ref64(mlp, cand[i][0])[0]
        torch.testing.assert_close(y_static[0].double(), want, rtol=TOL, atol=TOL)


def test_model_generates_on_mxfp4_experts(monkeypatch):
    calls = counted(monkeypatch)
    torch.manual_seed(0)
    model = models.build("moe-tiny").to(DEV).bfloat16()
    for buf in model.buffers():  # rope tables stay fp32
        buf.data = buf.data.float()
    ids = torch.randint(0, model.cfg.vocab_size, (2, 5), device=DEV)
    assert model.generate(ids, max_new_tokens=4, weight_quant="mxfp4").shape == (2, 9)
    assert not any(p.dim() == 3 for p in model.parameters())
    assert all(getattr(blk.mlp, n).dtype == torch.uint8
               for blk in model.blocks for n in MoEMLP._MXFP4_BUFFERS)
    # the prefill (10 tokens) and the 3 decode steps (2 tokens) each pass every layer once
    assert calls == [10] * model.cfg.n_layers + [2] * (3 * model.cfg.n_layers)
