"""Ragged batches on the GPU: per-sequence decode attention, per-sequence
row append, prefill with seq_lens, and the model / graphed-decoder routes
that use them (right-padded prompts, stop token)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hypha_amd import _C, models, ops
    from hypha_amd.models.kv_cache import KVCache

DEV = "cuda:0"
TOL = dict(rtol=2e-2, atol=2e-2)  # the project's attention-forward tolerance


def rand_bf16(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).bfloat16().to(DEV)


def i32(xs):
    return torch.tensor(xs, dtype=torch.int32, device=DEV)


def i64(xs):
    return torch.tensor(xs, dtype=torch.long, device=DEV)


def ids_of(shape):
    return "-".join(str(x) for x in shape[:-1]) + "-" + "_".join(map(str, shape[-1]))


# ---- decode kernel --------------------------------------------------------

# (B, Hq, Hkv, D, T_alloc, lens)
DECODE_SHAPES = [
    (4, 8, 2, 128, 300, [300, 1, 129, 0]),
    (3, 8, 8, 64, 130, [64, 65, 130]),
    (2, 8, 1, 64, 257, [257, 3]),
]


def decode_ref(q, k, v, t):
    """fp32 softmax attention of one sequence: q [Hq, D], k/v [t, Hkv, D]."""
    rep = q.shape[0] // k.shape[1]
    kh = k.float().permute(1, 0, 2).repeat_interleave(rep, dim=0)  # [Hq, t, D]
    vh = v.float().permute(1, 0, 2).repeat_interleave(rep, dim=0)
    scores = torch.einsum("hd,htd->ht", q.float(), kh) / q.shape[-1] ** 0.5
    return torch.einsum("ht,htd->hd", torch.softmax(scores, -1), vh)


@pytest.mark.parametrize("shape", DECODE_SHAPES, ids=ids_of)
def test_decode_varlen_kernel(shape):
    B, Hq, Hkv, D, T, lens = shape
    q = rand_bf16(B, Hq, D, seed=1)
    kc = rand_bf16(B, T, Hkv, D, seed=2)
    vc = rand_bf16(B, T, Hkv, D, seed=3)
    kn, vn = kc.clone(), vc.clone()
    for b, t in enumerate(lens):  # nothing past a sequence's length may be read
        kn[b, t:] = float("nan")
        vn[b, t:] = float("nan")
    o = ops.attn_decode_varlen(q, kn, vn, i32(lens))
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    for b, t in enumerate(lens):
        if t == 0:
            assert (o[b] == 0).all(), o[b]
            continue
        ref = decode_ref(q[b], kc[b, :t], vc[b, :t], t)
        print(f"{ids_of(shape)} b={b} t={t}: max abs err "
              f"{(o[b].float() - ref).abs().max().item():.3e}")
        torch.testing.assert_close(o[b].float(), ref, **TOL)
    # a tighter host bound only changes the split grid
    o2 = ops.attn_decode_varlen(q, kn, vn, i32(lens), max_len=max(lens))
    torch.testing.assert_close(o2.float(), o.float(), **TOL)

    # equal lengths: the single-length kernel's result
    t = max(lens)
    kn, vn = kc.clone(), vc.clone()
    kn[:, t:] = float("nan")
    vn[:, t:] = float("nan")
    same = ops.attn_decode_varlen(q, kn, vn, i32([t] * B), max_len=t)
    old = _C.attn_decode(q, kn, vn, t)
    print(f"{ids_of(shape)} equal lengths t={t}: bit-equal to attn_decode: "
          f"{torch.equal(same, old)}, max abs diff "
          f"{(same.float() - old.float()).abs().max().item():.3e}")
    torch.testing.assert_close(same.float(), old.float(), **TOL)


def test_decode_varlen_kernel_fp8():
    B, Hq, Hkv, D, T, lens = DECODE_SHAPES[0]
    q = rand_bf16(B, Hq, D, seed=4)
    cache = KVCache(B, T, Hkv, D, DEV, quant="fp8")
    cache.append(rand_bf16(B, T, Hkv, D, seed=5), rand_bf16(B, T, Hkv, D, seed=6))
    kd, vd = cache.dequant(T)  # quantisation error is common to both sides
    for b, t in enumerate(lens):  # NaN scales, NaN (0x7f) bytes past each length
        cache.k_scale[b, t:] = float("nan")
        cache.v_scale[b, t:] = float("nan")
        cache.k.view(torch.uint8)[b, t:] = 0x7F
        cache.v.view(torch.uint8)[b, t:] = 0x7F
    o = ops.attn_decode_varlen(q, cache.k, cache.v, i32(lens), cache.k_scale,
                               cache.v_scale)
    for b, t in enumerate(lens):
        if t == 0:
            assert (o[b] == 0).all(), o[b]
            continue
        ref = decode_ref(q[b], kd[b, :t], vd[b, :t], t)
        print(f"fp8 b={b} t={t}: max abs err {(o[b].float() - ref).abs().max().item():.3e}")
        torch.testing.assert_close(o[b].float(), ref, **TOL)


def test_decode_varlen_argument_checks():
    q = rand_bf16(2, 4, 64, seed=7)
    kc = rand_bf16(2, 16, 2, 64, seed=8)
    with pytest.raises(ValueError):  # int64 lengths
        ops.attn_decode_varlen(q, kc, kc, i64([3, 4]))
    with pytest.raises(ValueError):  # one length too few
        ops.attn_decode_varlen(q, kc, kc, i32([3]))
    with pytest.raises(ValueError):  # max_len past the cache
        ops.attn_decode_varlen(q, kc, kc, i32([3, 4]), max_len=17)
    with pytest.raises(RuntimeError):  # the same, at the extension boundary
        _C.attn_decode_varlen(q, kc, kc, i32([3]), 16)
    with pytest.raises(RuntimeError):
        _C.attn_decode_varlen(q, kc, kc, i32([3, 4]), 17)
    # lengths outside [0, T_alloc] are clamped, not followed
    o = ops.attn_decode_varlen(q, kc, kc, i32([-5, 99]))
    assert (o[0] == 0).all()
    torch.testing.assert_close(o[1:].float(), _C.attn_decode(q, kc, kc, 16)[1:].float(),
                               **TOL)


# ---- per-sequence row append ----------------------------------------------


@pytest.mark.parametrize("D", [64, 128])
def test_append_rows_bf16(D):
    B, Hkv, T = 3, 2, 16
    k, v = rand_bf16(B, 1, Hkv, D, seed=10), rand_bf16(B, 1, Hkv, D, seed=11)
    for pos, live in (([0, 15, 7], [0, 1, 2]), ([-1, 16, 3], [2])):
        cache = KVCache(B, T, Hkv, D, DEV)
        cache.k.copy_(rand_bf16(B, T, Hkv, D, seed=12))
        cache.v.copy_(rand_bf16(B, T, Hkv, D, seed=13))
        want_k, want_v = cache.k.clone(), cache.v.clone()
        for b in live:
            want_k[b, pos[b]] = k[b, 0]
            want_v[b, pos[b]] = v[b, 0]
        cache.append_rows(k, v, i64(pos))
        assert torch.equal(cache.k, want_k) and torch.equal(cache.v, want_v), pos
        assert cache.t == 0


@pytest.mark.parametrize("D", [64, 128])
def test_append_rows_fp8_bit_equal_to_single_position_append(D):
    B, Hkv, T = 3, 2, 16
    k, v = rand_bf16(B, 1, Hkv, D, seed=14), rand_bf16(B, 1, Hkv, D, seed=15)

    def parts(c):
        return [c.k.view(torch.uint8), c.v.view(torch.uint8), c.k_scale, c.v_scale]

    def fresh():
        c = KVCache(B, T, Hkv, D, DEV, quant="fp8")
        g = torch.Generator(device="cpu").manual_seed(16)
        for p in parts(c)[:2]:  # distinct bytes everywhere, so a stray write shows
            p.copy_(torch.randint(0, 0x7E, p.shape, generator=g, dtype=torch.uint8))
        c.k_scale.fill_(3.0)
        c.v_scale.fill_(5.0)
        return c

    for pos, live in (([0, 15, 7], [0, 1, 2]), ([-1, 16, 3], [2])):
        got = fresh()
        got.append_rows(k, v, i64(pos))
        want = fresh()
        for b in live:  # what the existing kernel writes for that row, there
            scratch = fresh()
            _C.kv_append_fp8_(k, v, scratch.k, scratch.v, scratch.k_scale,
                              scratch.v_scale, i64([pos[b]]))
            for w, s in zip(parts(want), parts(scratch)):
                w[b, pos[b]] = s[b, pos[b]]
        for name, g, w in zip(("k", "v", "k_scale", "v_scale"), parts(got), parts(want)):
            assert torch.equal(g, w), (pos, name)


@pytest.mark.parametrize("D", [64, 128])
def test_append_kernel_writes_the_cache_quantisers_bytes(D):
    """A decoded row must be the same row whichever path appended it: the
    kernel's bytes and scales are those of KVCache._quantize_rows (the PyTorch
    path of the uniform eager loop), bit for bit. 4096 rows per head dim:
    reciprocal-multiply instead of division shows in about 2% of rows."""
    B, Hkv, T = 256, 8, 4
    k, v = rand_bf16(B, 1, Hkv, D, seed=17), rand_bf16(B, 1, Hkv, D, seed=18)
    cache = KVCache(B, T, Hkv, D, DEV, quant="fp8")
    pos = torch.arange(B, device=DEV) % T
    cache.append_rows(k, v, pos)
    single = KVCache(B, T, Hkv, D, DEV, quant="fp8")
    _C.kv_append_fp8_(k, v, single.k, single.v, single.k_scale, single.v_scale, i64([2]))
    rows = torch.arange(B, device=DEV)
    for x, c8, cs, s8, ss in ((k, cache.k, cache.k_scale, single.k, single.k_scale),
                              (v, cache.v, cache.v_scale, single.v, single.v_scale)):
        q, scale = cache._quantize_rows(x)  # [B, 1, Hkv, D], [B, 1, Hkv]
        want8, want_s = q.view(torch.uint8)[:, 0], scale[:, 0]
        got8 = c8.view(torch.uint8)[rows, pos]
        bad = (got8 != want8).any(-1).sum().item()
        print(f"D={D}: rows with another byte {bad}, another scale "
              f"{(cs[rows, pos] != want_s).sum().item()} of {B * Hkv}")
        assert torch.equal(cs[rows, pos], want_s)
        assert torch.equal(got8, want8)
        assert torch.equal(ss[:, 2], want_s) and torch.equal(s8.view(torch.uint8)[:, 2], want8)


# ---- prefill with seq_lens ------------------------------------------------

# (B, Hq, Hkv, D, pos, s, T_alloc, seq_lens)
PREFILL_SHAPES = [
    (3, 8, 2, 128, 0, 200, 200, [200, 12, 129]),
    (2, 4, 2, 64, 100, 77, 256, [177, 100]),
    (2, 4, 2, 64, 100, 77, 256, [150, 101]),
]


def _check_prefill(o, q, kd, vd, pos, lens, tag):
    s = q.shape[1]
    for b, n in enumerate(lens):
        live = max(0, min(n, pos + s) - pos)
        assert (o[b, live:] == 0).all(), (tag, b)  # dead rows: exact zeros
        if live == 0:
            continue
        sl = slice(b, b + 1)
        ref = ops.reference.attention_cached(q[sl, :live].float(), kd[sl, :n].float(),
                                             vd[sl, :n].float(), pos)
        print(f"{tag} b={b} live={live}: max abs err "
              f"{(o[sl, :live].float() - ref).abs().max().item():.3e}")
        torch.testing.assert_close(o[sl, :live].float(), ref, **TOL)


@pytest.mark.parametrize("shape", PREFILL_SHAPES, ids=ids_of)
def test_prefill_seq_lens_kernel(shape):
    B, Hq, Hkv, D, pos, s, T, lens = shape
    q = rand_bf16(B, s, Hq, D, seed=20)
    kc = rand_bf16(B, T, Hkv, D, seed=21)
    vc = rand_bf16(B, T, Hkv, D, seed=22)
    kn, vn = kc.clone(), vc.clone()
    for b, n in enumerate(lens):
        kn[b, n:] = float("nan")
        vn[b, n:] = float("nan")
    o = ops.attn_prefill(q, kn, vn, pos, seq_lens=i32(lens))
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    _check_prefill(o, q, kc, vc, pos, lens, ids_of(shape))


def test_prefill_seq_lens_kernel_fp8():
    B, Hq, Hkv, D, pos, s, T, lens = PREFILL_SHAPES[2]
    q = rand_bf16(B, s, Hq, D, seed=23)
    cache = KVCache(B, T, Hkv, D, DEV, quant="fp8")
    cache.append(rand_bf16(B, T, Hkv, D, seed=24), rand_bf16(B, T, Hkv, D, seed=25))
    kd, vd = cache.dequant(T)
    for b, n in enumerate(lens):
        cache.k_scale[b, n:] = float("nan")
        cache.v_scale[b, n:] = float("nan")
        cache.k.view(torch.uint8)[b, n:] = 0x7F
        cache.v.view(torch.uint8)[b, n:] = 0x7F
    o = ops.attn_prefill(q, cache.k, cache.v, pos, cache.k_scale, cache.v_scale,
                         seq_lens=i32(lens))
    _check_prefill(o, q, kd, vd, pos, lens, "fp8 " + ids_of(PREFILL_SHAPES[2]))


def test_prefill_seq_lens_full_lengths_equal_plain_prefill():
    B, Hq, Hkv, D, pos, s, T = 2, 8, 2, 128, 100, 77, 256
    q = rand_bf16(B, s, Hq, D, seed=26)
    kc = rand_bf16(B, T, Hkv, D, seed=27)
    vc = rand_bf16(B, T, Hkv, D, seed=28)
    plain = ops.attn_prefill(q, kc, vc, pos)
    # lengths past the chunk are clamped to pos + s
    full = ops.attn_prefill(q, kc, vc, pos, seq_lens=i32([pos + s, 10_000]))
    assert torch.equal(plain, full)
    with pytest.raises(ValueError):
        ops.attn_prefill(q, kc, vc, pos, seq_lens=i64([pos + s, pos + s]))
    with pytest.raises(RuntimeError):
        _C.attn_prefill_varlen(q, kc, kc, pos, i32([pos + s]))


def test_apply_rope_qk_at_kernel():
    B, Hq, Hkv, D = 3, 8, 2, 128
    cos, sin = ops.reference.rope_cos_sin(64, D, 10000.0)
    cos, sin = cos.to(DEV), sin.to(DEV)
    q, k = rand_bf16(B, 1, Hq, D, seed=30), rand_bf16(B, 1, Hkv, D, seed=31)
    positions = [9, 0, 63]
    qo, ko = ops.apply_rope_qk_at(q, k, cos, sin, i64(positions))
    for b, p in enumerate(positions):  # the existing single-position call, bit for bit
        qr, kr = ops.apply_rope_qk(q[b:b + 1], k[b:b + 1], cos[p:p + 1], sin[p:p + 1],
                                   layout="bshd")
        assert torch.equal(qo[b:b + 1], qr) and torch.equal(ko[b:b + 1], kr), b


# ---- model ----------------------------------------------------------------


def _bf16_model(name, **kw):
    model = models.build(name, **kw).to(DEV).bfloat16().eval()
    for buf in model.buffers():  # rope tables stay fp32
        if buf.dtype is torch.bfloat16:
            buf.data = buf.data.float()
    return model


def _valid_agreement(tokens, lens, refs):
    """Fraction of equal tokens, pooled over every sequence's valid tokens
    (the existing generation tests pool their whole batch the same way)."""
    eq = torch.cat([(tokens[b, :n] == refs[b][:n]).float()
                    for b, n in enumerate(lens)])
    return eq.mean().item()


@pytest.mark.parametrize("kw", [{}, {"kv_quant": "fp8"}, {"prefill_chunk": 16}],
                         ids=["bf16", "fp8", "chunk16"])
def test_generate_ragged_matches_batch1_runs(monkeypatch, kw):
    """Each sequence of a right-padded batch against its own batch-1 run; the
    reference attention is patched to raise, so every pass is native. Bar:
    0.95 agreement pooled over the valid tokens, as the existing bf16
    generation tests pool their batch (a per-sequence bar would demand exact
    equality of the 13-token sequence, which bf16 GEMMs of different M do not
    promise).

    Measured on an MI355X: 1.000 (new tokens 1.000) for bf16, fp8 and
    chunk16. The fp8 case first reached 0.942: kv_append_fp8_kernel then
    computed x * (1 / scale) with scale = amax / 448, which is not what
    KVCache._quantize_rows computes, and one differing byte decided a one-ulp
    logit tie in the 5-token sequence. The kernel now writes the cache
    quantiser's bytes (test_append_kernel_writes_the_cache_quantisers_bytes)."""
    def boom(*a, **k):
        raise AssertionError("reference.attention_cached hit on the GPU path")

    monkeypatch.setattr(ops.reference, "attention_cached", boom)
    torch.manual_seed(17)
    model = _bf16_model("llama-tiny")
    lens, s, new = [37, 5, 20], 37, 8
    ids = torch.randint(0, 256, (3, s), device=DEV)
    pad = int(ids[0, 3])
    for b, n in enumerate(lens):
        ids[b, n:] = pad
    tokens, out_lens = model.generate(ids, max_new_tokens=new, prompt_lens=lens,
                                      pad_token_id=pad, **kw)
    assert tokens.shape == (3, s + new)
    assert out_lens.tolist() == [n + new for n in lens]
    refs = [model.generate(ids[b:b + 1, :n], max_new_tokens=new, **kw)[0]
            for b, n in enumerate(lens)]
    for b, n in enumerate(lens):
        assert torch.equal(tokens[b, :n], ids[b, :n])
        assert (tokens[b, n + new:] == pad).all()
    agree = _valid_agreement(tokens, out_lens.tolist(), refs)
    new_agree = torch.cat([(tokens[b, n:n + new] == refs[b][n:]).float()
                           for b, n in enumerate(lens)]).mean().item()
    print(f"ragged {kw}: agreement {agree:.3f}, new tokens {new_agree:.3f}")
    assert agree >= 0.95, (agree, tokens, refs)


def _pick_stop(tokens, lens, new, pad):
    """(b, step, id): a token sequence b first emits at a step that is neither
    the first nor the last, and that some other sequence never emits."""
    gen = [tokens[b, n:n + new].tolist() for b, n in enumerate(lens)]
    for b, toks in enumerate(gen):
        for step in range(1, new - 1):
            e = toks[step]
            if e == pad or e in toks[:step]:
                continue
            if any(e not in other for o, other in enumerate(gen) if o != b):
                return b, step, e
    raise AssertionError(f"no usable stop token in {gen}")


def test_graphed_decoder_ragged():
    from hypha_amd.runtime.graphed_decode import GraphedDecoder

    torch.manual_seed(29)
    model = _bf16_model("llama-tiny", hidden_size=2048, n_heads=16, n_kv_heads=4,
                        ffn_hidden=4096, n_layers=2)
    lens, s, new, pad = [128, 70, 3, 97], 128, 24, 0
    ids = torch.randint(1, 500, (4, s), device=DEV)
    for b, n in enumerate(lens):
        ids[b, n:] = pad
    dec = GraphedDecoder(model, batch=4, prompt_len=s, max_new=32)
    uniform_before = dec.generate(ids, max_new_tokens=new)

    eager, eager_lens = model.generate(ids, max_new_tokens=new, prompt_lens=lens)
    graphed, g_lens = dec.generate(ids, max_new_tokens=new, prompt_lens=lens)
    assert dec.graph_r is not None  # really captured
    assert graphed.shape == eager.shape == (4, s + new)
    assert g_lens.tolist() == eager_lens.tolist() == [n + new for n in lens]
    agree = _valid_agreement(graphed, g_lens.tolist(), list(eager))
    print(f"graphed ragged vs eager ragged: agreement {agree:.3f}")
    assert agree >= 0.97, (agree, graphed, eager)
    for b, n in enumerate(lens):
        assert (graphed[b, n + new:] == pad).all()

    # second call replays the captured graph
    graphed2, g_lens2 = dec.generate(ids, max_new_tokens=new, prompt_lens=lens)
    assert torch.equal(graphed2, graphed) and torch.equal(g_lens2, g_lens)

    # the uniform graph and its state are untouched by the ragged one
    assert torch.equal(dec.generate(ids, max_new_tokens=new), uniform_before)

    # stop token: the finished sequence is padded and its length frozen
    b_stop, step, eos = _pick_stop(graphed, lens, new, pad)
    stopped, s_lens = dec.generate(ids, max_new_tokens=new, prompt_lens=lens,
                                   eos_token_id=eos)
    n = lens[b_stop]
    assert s_lens[b_stop].item() == n + step + 1
    assert torch.equal(stopped[b_stop, :n + step + 1], graphed[b_stop, :n + step + 1])
    assert stopped[b_stop, n + step].item() == eos
    assert (stopped[b_stop, n + step + 1:] == pad).all()
    others = [b for b in range(4) if eos not in graphed[b, lens[b]:lens[b] + new].tolist()]
    assert others
    for b in others:
        assert s_lens[b].item() == lens[b] + new
