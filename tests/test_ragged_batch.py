"""Ragged batches on the CPU reference path (fp32, llama-tiny): a right-padded
batch with per-sequence lengths must generate what each prompt generates on
its own through the existing single-length path, a stop token must freeze
one sequence without disturbing the others, and the per-sequence reference
ops must equal slicing and looping over the single-length ones."""

import pytest
import torch

from hypha_amd import models, ops
from hypha_amd.models.kv_cache import KVCache

LENS = [5, 12, 1]
S = 12
NEW = 6
SEED = 3


@pytest.fixture(scope="module")
def setup():
    """Model, right-padded batch and the per-sequence reference runs (shared,
    never modified)."""
    torch.manual_seed(SEED)
    model = models.build("llama-tiny").eval()
    prompts = torch.randint(0, 512, (3, S))
    pad = int(prompts[1, 3])  # a pad id that also occurs inside a prompt
    ids = prompts.clone()
    for b, n in enumerate(LENS):
        ids[b, n:] = pad
    refs = {}
    for kw_key, kw in (("plain", {}), ("fp8", {"kv_quant": "fp8"})):
        refs[kw_key] = [model.generate(ids[b:b + 1, :n], max_new_tokens=NEW, **kw)[0]
                        for b, n in enumerate(LENS)]
    return model, ids, pad, refs


def _check_against(tokens, lens, refs, pad):
    assert tokens.shape == (3, S + NEW)
    assert lens.tolist() == [n + NEW for n in LENS]
    for b, n in enumerate(LENS):
        assert torch.equal(tokens[b, :n + NEW], refs[b]), (b, tokens[b], refs[b])
        assert (tokens[b, n + NEW:] == pad).all()


@pytest.mark.parametrize("kw,ref_key", [({}, "plain"), ({"prefill_chunk": 4}, "plain"),
                                        ({"kv_quant": "fp8"}, "fp8")],
                         ids=["one-pass", "chunk4", "fp8"])
def test_ragged_batch_equals_per_sequence_runs(setup, kw, ref_key):
    model, ids, pad, refs = setup
    assert (ids[1, :LENS[1]] == pad).any()  # the pad id is a real prompt token too
    tokens, lens = model.generate(ids, max_new_tokens=NEW, prompt_lens=LENS,
                                  pad_token_id=pad, **kw)
    _check_against(tokens, lens, refs[ref_key], pad)
    # lengths given as a tensor behave the same
    tokens_t, lens_t = model.generate(ids, max_new_tokens=NEW,
                                      prompt_lens=torch.tensor(LENS),
                                      pad_token_id=pad, **kw)
    assert torch.equal(tokens_t, tokens) and torch.equal(lens_t, lens)


def _pick_stop(refs):
    """A token some sequence first emits at a step that is neither the first
    nor the last, and that at least one other sequence never emits."""
    new = [refs[b][n:].tolist() for b, n in enumerate(LENS)]
    for b, toks in enumerate(new):
        for step in range(1, NEW - 1):
            e = toks[step]
            if e in toks[:step]:
                continue
            if any(e not in other for o, other in enumerate(new) if o != b):
                return b, step, e
    raise AssertionError(f"seed {SEED} gives no usable stop token: {new}")


def test_stop_token_freezes_one_sequence(setup):
    model, ids, pad, refs = setup
    refs = refs["plain"]
    b_stop, step, eos = _pick_stop(refs)
    assert eos != pad
    tokens, lens = model.generate(ids, max_new_tokens=NEW, prompt_lens=LENS,
                                  eos_token_id=eos, pad_token_id=pad)
    n = LENS[b_stop]
    assert lens[b_stop].item() == n + step + 1          # frozen at the stop token
    assert tokens[b_stop, n + step].item() == eos        # which it keeps
    assert torch.equal(tokens[b_stop, :n + step + 1], refs[b_stop][:n + step + 1])
    assert (tokens[b_stop, n + step + 1:] == pad).all()  # padded afterwards
    untouched = 0
    for b, n in enumerate(LENS):
        new = refs[b][n:].tolist()
        keep = new.index(eos) + 1 if eos in new else NEW
        untouched += eos not in new
        assert lens[b].item() == n + keep
        assert torch.equal(tokens[b, :n + keep], refs[b][:n + keep])
        assert (tokens[b, n + keep:] == pad).all()
    assert untouched >= 1

    # without prompt_lens: tokens only, pads after the stop token
    full = model.generate(ids[:, :5], max_new_tokens=NEW)
    e2 = int(full[0, 5 + 2])
    out = model.generate(ids[:, :5], max_new_tokens=NEW, eos_token_id=e2, pad_token_id=pad)
    assert isinstance(out, torch.Tensor) and out.shape == full.shape
    for b in range(3):
        new = full[b, 5:].tolist()
        keep = new.index(e2) + 1 if e2 in new else NEW
        assert torch.equal(out[b, :5 + keep], full[b, :5 + keep])
        assert (out[b, 5 + keep:] == pad).all()


def test_prompt_lens_argument_checks(setup):
    model, ids, pad, _ = setup
    with pytest.raises(ValueError):  # wrong size
        model.generate(ids, max_new_tokens=2, prompt_lens=[5, 12])
    with pytest.raises(ValueError):  # L_b = 0
        model.generate(ids, max_new_tokens=2, prompt_lens=[5, 0, 1])
    with pytest.raises(ValueError):  # L_b > s
        model.generate(ids, max_new_tokens=2, prompt_lens=[5, 13, 1])


# ---- reference paths of the per-sequence ops ------------------------------


def _rand(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


@pytest.mark.parametrize("quant", [None, "fp8"])
def test_attn_decode_varlen_reference(quant):
    B, Hq, Hkv, D, T = 4, 4, 2, 16, 20
    lens = [20, 1, 7, 0]
    q = _rand(B, Hq, D, seed=1)
    cache = KVCache(B, T, Hkv, D, "cpu", dtype=torch.float32, quant=quant)
    cache.append(_rand(B, T, Hkv, D, seed=2), _rand(B, T, Hkv, D, seed=3))
    o = ops.attn_decode_varlen(q, cache.k, cache.v, torch.tensor(lens, dtype=torch.int32),
                               cache.k_scale, cache.v_scale)
    for b, t in enumerate(lens):
        if t == 0:
            assert (o[b] == 0).all()
            continue
        sl = slice(b, b + 1)
        ref = ops.attn_decode(q[sl], cache.k[sl], cache.v[sl], t,
                              None if quant is None else cache.k_scale[sl],
                              None if quant is None else cache.v_scale[sl])
        torch.testing.assert_close(o[sl], ref, rtol=0, atol=0)
    with pytest.raises(ValueError):
        ops.attn_decode_varlen(q, cache.k, cache.v, torch.tensor(lens), cache.k_scale,
                               cache.v_scale)  # int64 lengths


@pytest.mark.parametrize("quant", [None, "fp8"])
def test_append_rows_reference(quant):
    B, Hkv, D, T = 3, 2, 16, 8
    k, v = _rand(B, 1, Hkv, D, seed=4), _rand(B, 1, Hkv, D, seed=5)

    def fresh():
        return KVCache(B, T, Hkv, D, "cpu", dtype=torch.float32, quant=quant)

    def state(c):
        parts = [c.k, c.v] + ([] if quant is None else [c.k_scale, c.v_scale])
        return [p.view(torch.uint8).clone() if p.dtype == torch.float8_e4m3fn else p.clone()
                for p in parts]

    for pos in ([0, 7, 3], [-1, 8, 3]):
        got = fresh()
        got.append_rows(k, v, torch.tensor(pos))
        want = fresh()
        for b, p in enumerate(pos):  # the single-position append, one sequence at a time
            if not 0 <= p < T:
                continue
            one = fresh()
            one.append_at(k[b:b + 1].expand(B, -1, -1, -1).contiguous(),
                          v[b:b + 1].expand(B, -1, -1, -1).contiguous(), torch.tensor([p]))
            want.k.view(torch.uint8)[b, p] = one.k.view(torch.uint8)[b, p]
            want.v.view(torch.uint8)[b, p] = one.v.view(torch.uint8)[b, p]
            if quant is not None:
                want.k_scale[b, p] = one.k_scale[b, p]
                want.v_scale[b, p] = one.v_scale[b, p]
        for g, w in zip(state(got), state(want)):
            assert torch.equal(g, w), pos
        assert got.t == 0  # like append_at, the counter does not move


def test_apply_rope_qk_at_reference():
    B, Hq, Hkv, D = 3, 4, 2, 16
    cos, sin = ops.reference.rope_cos_sin(32, D, 10000.0)
    q, k = _rand(B, 1, Hq, D, seed=6), _rand(B, 1, Hkv, D, seed=7)
    positions = [9, 0, 31]
    qo, ko = ops.apply_rope_qk_at(q, k, cos, sin, torch.tensor(positions))
    for b, p in enumerate(positions):
        qr, kr = ops.apply_rope_qk(q[b:b + 1], k[b:b + 1], cos[p:], sin[p:], layout="bshd")
        assert torch.equal(qo[b:b + 1], qr) and torch.equal(ko[b:b + 1], kr)


@pytest.mark.parametrize("quant", [None, "fp8"])
@pytest.mark.parametrize("pos,s,lens", [(0, 10, [10, 3, 7]), (6, 5, [11, 6, 8]),
                                        (6, 5, [9, 4, 7])])
def test_attn_prefill_seq_lens_reference(quant, pos, s, lens):
    B, Hq, Hkv, D, T = 3, 4, 2, 16, 12
    q = _rand(B, s, Hq, D, seed=8)
    cache = KVCache(B, T, Hkv, D, "cpu", dtype=torch.float32, quant=quant)
    cache.append(_rand(B, T, Hkv, D, seed=9), _rand(B, T, Hkv, D, seed=10))
    scales = {} if quant is None else dict(kscale=cache.k_scale.clone(),
                                           vscale=cache.v_scale.clone())
    kc, vc = cache.k.clone(), cache.v.clone()
    want = []
    for b, n in enumerate(lens):  # slices of the single-length reference
        live = max(0, min(n, pos + s) - pos)
        row = torch.zeros(1, s, Hq, D)
        if live:
            sl = slice(b, b + 1)
            sc = {key: val[sl] for key, val in scales.items()}
            row[:, :live] = ops.attn_prefill(q[sl, :live], kc[sl], vc[sl], pos, **sc)
        want.append(row)
    # what lies past each length must not matter
    for b, n in enumerate(lens):
        if quant is None:
            kc[b, n:] = float("nan")
            vc[b, n:] = float("nan")
        else:
            scales["kscale"][b, n:] = float("nan")
            scales["vscale"][b, n:] = float("nan")
    o = ops.attn_prefill(q, kc, vc, pos, seq_lens=torch.tensor(lens, dtype=torch.int32),
                         **scales)
    want = torch.cat(want)
    torch.testing.assert_close(o, want, rtol=1e-5, atol=1e-6)
    for b, n in enumerate(lens):
        assert (o[b, max(0, n - pos):] == 0).all()
