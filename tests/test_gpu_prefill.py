"""Native prefill attention over the KV cache (ops/hip/prefill.hip): ragged
prompts, chunked continuation, bf16 and fp8 caches, and the model-level
routes that reach it."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hypha_amd import _C, models, ops
    from hypha_amd.models.kv_cache import KVCache

DEV = "cuda:0"
TOL = dict(rtol=2e-2, atol=2e-2)  # the project's attention-forward tolerance

# (B, Hq, Hkv, D, pos, s, T_alloc)
SHAPES = [
    (2, 8, 2, 128, 0, 12, 40),      # < one wave; B=2: tail store must not leak
    (2, 4, 4, 64, 0, 200, 200),     # 2 workgroups, ragged q tail, T_alloc == t
    (2, 8, 2, 128, 100, 77, 256),   # offset no multiple of 32/64
    (1, 8, 1, 64, 130, 130, 260),   # GQA group 8, 2 workgroups, all ragged
    (1, 4, 2, 128, 128, 128, 256),  # aligned continuation
    (2, 4, 2, 64, 63, 2, 65),       # smallest chunk across a tile boundary
]


def rand_bf16(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).bfloat16().to(DEV)


def ref_fp32(q, k, v, pos):
    """fp32 masked softmax on the same (bf16-valued) inputs."""
    return ops.reference.attention_cached(q.float(), k.float(), v.float(), pos)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_prefill_kernel_vs_fp32_reference(shape):
    B, Hq, Hkv, D, pos, s, T_alloc = shape
    t = pos + s
    q = rand_bf16(B, s, Hq, D, seed=1)
    kc = rand_bf16(B, T_alloc, Hkv, D, seed=2)
    vc = rand_bf16(B, T_alloc, Hkv, D, seed=3)
    kc[:, t:] = float("nan")  # the stale tail must never reach the output
    vc[:, t:] = float("nan")
    o = ops.attn_prefill(q, kc, vc, pos)
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    ref = ref_fp32(q, kc[:, :t], vc[:, :t], pos)
    print(f"{shape}: max abs err {(o.float() - ref).abs().max().item():.3e}")
    torch.testing.assert_close(o.float(), ref, **TOL)


@pytest.mark.parametrize("shape", SHAPES[2:4], ids=lambda s: "-".join(map(str, s)))
def test_prefill_kernel_fp8_cache(shape):
    B, Hq, Hkv, D, pos, s, T_alloc = shape
    t = pos + s
    q = rand_bf16(B, s, Hq, D, seed=4)
    cache = KVCache(B, T_alloc, Hkv, D, DEV, quant="fp8")
    cache.append(rand_bf16(B, t, Hkv, D, seed=5), rand_bf16(B, t, Hkv, D, seed=6))
    # poison everything past the valid length: NaN scales, NaN (0x7f) bytes
    cache.k_scale[:, t:] = float("nan")
    cache.v_scale[:, t:] = float("nan")
    cache.k.view(torch.uint8)[:, t:] = 0x7F
    cache.v.view(torch.uint8)[:, t:] = 0x7F
    o = ops.attn_prefill(q, cache.k, cache.v, pos, cache.k_scale, cache.v_scale)
    kd, vd = cache.dequant(t)  # quantisation error is common to both sides
    ref = ref_fp32(q, kd, vd, pos)
    print(f"fp8 {shape}: max abs err {(o.float() - ref).abs().max().item():.3e}")
    torch.testing.assert_close(o.float(), ref, **TOL)


def test_prefill_chunks_match_one_shot_flash_kernel():
    B, Hq, Hkv, D, S = 2, 8, 2, 128, 256
    q = rand_bf16(B, S, Hq, D, seed=7)
    k = rand_bf16(B, S, Hkv, D, seed=8)
    v = rand_bf16(B, S, Hkv, D, seed=9)
    ref = ops.flash_attention(q, k, v, causal=True, layout="bshd")
    pos = 0
    for n in (96, 96, 64):
        o = ops.attn_prefill(q[:, pos:pos + n].contiguous(), k, v, pos)
        torch.testing.assert_close(o.float(), ref[:, pos:pos + n].float(), **TOL)
        pos += n
    assert pos == S


@pytest.mark.parametrize("shape", [(2, 8, 2, 128), (1, 4, 4, 64)],
                         ids=lambda s: "-".join(map(str, s)))
def test_prefill_aligned_equals_flash_kernel(shape):
    """pos = 0, s = T_alloc = 256: no tail, no offset. Both kernels then run
    the one shared tile step (attn_tile.h) over the same tiles."""
    B, Hq, Hkv, D = shape
    S = 256
    q = rand_bf16(B, S, Hq, D, seed=10)
    k = rand_bf16(B, S, Hkv, D, seed=11)
    v = rand_bf16(B, S, Hkv, D, seed=12)
    o = ops.attn_prefill(q, k, v, 0)
    ref = ops.flash_attention(q, k, v, causal=True, layout="bshd")
    print(f"{shape}: bit-equal to the flash kernel: {torch.equal(o, ref)}, "
          f"max abs diff {(o.float() - ref.float()).abs().max().item():.3e}")
    torch.testing.assert_close(o.float(), ref.float(), **TOL)


def _bf16_model(name):
    model = models.build(name).to(DEV).bfloat16().eval()
    for buf in model.buffers():  # rope tables stay fp32
        if buf.dtype is torch.bfloat16:
            buf.data = buf.data.float()
    return model


def _no_reference(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("reference.attention_cached hit on the GPU path")

    monkeypatch.setattr(ops.reference, "attention_cached", boom)


@pytest.mark.parametrize("name,kw", [("llama-tiny", {}), ("gpt2-small", {}),
                                     ("moe-tiny", {}),
                                     ("llama-tiny", {"kv_quant": "fp8"})],
                         ids=["llama", "gpt2", "moe", "llama-fp8"])
def test_generate_chunked_prefill_matches_one_shot(monkeypatch, name, kw):
    """37-token prompt (ragged), chunks of 16: every prefill pass runs the
    native kernel (the reference is patched to raise) and greedy tokens agree
    with the single-pass run at the project's bar for bf16 generation."""
    _no_reference(monkeypatch)
    torch.manual_seed(17)
    model = _bf16_model(name)
    ids = torch.randint(0, 256, (2, 37), device=DEV)
    one = model.generate(ids, max_new_tokens=8, **kw)
    chunked = model.generate(ids, max_new_tokens=8, prefill_chunk=16, **kw)
    assert one.shape == chunked.shape == (2, 45)
    agree = (one == chunked).float().mean().item()
    print(f"{name} {kw}: agreement {agree:.3f}, new tokens "
          f"{(one[:, 37:] == chunked[:, 37:]).float().mean().item():.3f}")
    assert agree >= 0.95, (name, agree, one[:, 37:], chunked[:, 37:])


def test_graphed_decoder_chunked_prefill(monkeypatch):
    from hypha_amd.runtime.graphed_decode import GraphedDecoder

    _no_reference(monkeypatch)
    torch.manual_seed(19)
    model = _bf16_model("llama-tiny")
    ids = torch.randint(0, 256, (2, 37), device=DEV)
    dec = GraphedDecoder(model, batch=2, prompt_len=37, max_new=4)
    one = dec.generate(ids, max_new_tokens=4)  # < 8 new tokens: eager steps
    chunked = dec.generate(ids, max_new_tokens=4, prefill_chunk=16)
    assert one.shape == chunked.shape == (2, 41)
    assert (one == chunked).float().mean().item() >= 0.95
    with pytest.raises(ValueError):
        dec.generate(ids, max_new_tokens=4, prefill_chunk=0)


def test_prefill_argument_checks():
    q = rand_bf16(1, 8, 4, 64, seed=10)
    kc = rand_bf16(1, 16, 2, 64, seed=11)
    with pytest.raises((RuntimeError, TypeError, ValueError)):  # wrong q dtype
        ops.attn_prefill(q.half(), kc, kc, 0)
    with pytest.raises((RuntimeError, TypeError, ValueError)):  # wrong cache dtype
        _C.attn_prefill(q, kc.half(), kc.half(), 0)
    with pytest.raises(ValueError):  # pos + s > T_alloc
        ops.attn_prefill(q, kc, kc, 9)
    with pytest.raises(RuntimeError):  # the same, at the extension boundary
        _C.attn_prefill(q, kc, kc, 9)
    q32 = rand_bf16(1, 8, 4, 32, seed=12)
    kc32 = rand_bf16(1, 16, 2, 32, seed=13)
    with pytest.raises(RuntimeError):  # unsupported head dim
        _C.attn_prefill(q32, kc32, kc32, 0)
    with pytest.raises(RuntimeError):  # Hq not a multiple of Hkv
        _C.attn_prefill(rand_bf16(1, 8, 3, 64, seed=14), kc, kc, 0)
    cache = KVCache(1, 16, 2, 64, DEV, quant="fp8")
    with pytest.raises(ValueError):  # fp8 cache without scales
        ops.attn_prefill(q, cache.k, cache.v, 0)
    with pytest.raises(RuntimeError):  # scales of the wrong shape
        _C.attn_prefill_fp8(q, cache.k, cache.v, cache.k_scale[:, :8].contiguous(),
                            cache.v_scale, 0)
