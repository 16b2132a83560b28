"""Paged KV cache on the GPU: the block-table decode, prefill and append
kernels against the contiguous kernels on the gathered cache (bit for bit:
the kernel bodies are shared and nothing in their arithmetic order depends on
addresses), and the model / graphed-decoder routes that use them.

In every kernel test the table is a scattered, interleaved assignment over a
pool with more pages than are used, and every row no sequence owns is poison
(bf16: NaN; fp8: byte 0x7F with NaN scales): unallocated pages and the rows
past a sequence's length in its last page."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hypha_amd import models, ops
    from hypha_amd.models.kv_cache import KVCache
    from hypha_amd.models.paged_kv import PAGE, PagePoolExhausted
    from hypha_amd.ops.interface import _attention_cached_varlen
    from hypha_amd.ops.reference import gather_pages

DEV = "cuda:0"
TOL = dict(rtol=2e-2, atol=2e-2)  # the project's attention-forward tolerance
EXTRA = 5  # pool pages no table names


def rand_bf16(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).bfloat16().to(DEV)


def i32(xs):
    return torch.tensor(xs, dtype=torch.int32, device=DEV)


def i64(xs):
    return torch.tensor(xs, dtype=torch.long, device=DEV)


def ids_of(shape):
    return "-".join("_".join(map(str, x)) if isinstance(x, list) else str(x)
                    for x in shape)


def scattered(n):
    return [p for p in range(n - 1, -1, -1) if p % 2 == 0] + \
           [p for p in range(n) if p % 2 == 1]


def make_table(rows, max_pages):
    """Interleaved, scattered table: slot j of sequence b (while b owns a
    j-th page) is perm[j * B + b]; the other slots are -1. Returns
    (table int32 [B, max_pages] on the device, n_pages)."""
    B = len(rows)
    n_pages = B * max_pages + EXTRA
    perm = scattered(n_pages)
    table = torch.full((B, max_pages), -1, dtype=torch.int32)
    for b, n in enumerate(rows):
        for j in range((n + PAGE - 1) // PAGE):
            table[b, j] = perm[j * B + b]
    return table.to(DEV), n_pages


def poisoned(n_pages, like):
    """A pool [n_pages, 64, ...] of poison in like's dtype."""
    shape = (n_pages, PAGE, *like.shape[2:])
    if like.dtype == torch.float8_e4m3fn:
        return torch.full(shape, 0x7F, dtype=torch.uint8, device=DEV).view(like.dtype)
    return torch.full(shape, float("nan"), dtype=like.dtype, device=DEV)


def scatter_rows(dense, table, rows, n_pages):
    """Pool holding dense[b, :rows[b]] ([B, T, ...]) at the table's pages,
    poison everywhere else."""
    pool = poisoned(n_pages, dense)
    raw = pool.view(torch.uint8) if pool.dtype == torch.float8_e4m3fn else pool
    src = dense.view(torch.uint8) if pool.dtype == torch.float8_e4m3fn else dense
    host = table.cpu()
    for b, n in enumerate(rows):
        for j in range((n + PAGE - 1) // PAGE):
            r = min(PAGE, n - j * PAGE)
            raw[int(host[b, j]), :r] = src[b, j * PAGE:j * PAGE + r]
    return pool


def same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def decode_ref(q, k, v):
    """fp32 softmax attention of one sequence: q [Hq, D], k/v [t, Hkv, D]."""
    rep = q.shape[0] // k.shape[1]
    kh = k.float().permute(1, 0, 2).repeat_interleave(rep, dim=0)  # [Hq, t, D]
    vh = v.float().permute(1, 0, 2).repeat_interleave(rep, dim=0)
    scores = torch.einsum("hd,htd->ht", q.float(), kh) / q.shape[-1] ** 0.5
    return torch.einsum("ht,htd->hd", torch.softmax(scores, -1), vh)


# ---- decode kernel --------------------------------------------------------

# (B, Hq, Hkv, D, max_pages, lens)
DECODE_SHAPES = [
    (4, 8, 2, 128, 5, [300, 1, 129, 0]),
    (3, 8, 8, 64, 3, [64, 65, 130]),  # page boundary
    (2, 8, 1, 64, 5, [257, 3]),
]


def _check_decode(tag, q, pools, scales, table, n_pages, lens, kd, vd):
    """pools/scales: (k, v) pools and (kscale, vscale) or (None, None);
    kd, vd: the clean logical cache in bf16 for the fp32 reference."""
    kp, vp = pools
    ks, vs = scales
    max_pages = table.shape[1]
    gk, gv = gather_pages(kp, table), gather_pages(vp, table)
    gks = gather_pages(ks, table) if ks is not None else None
    gvs = gather_pages(vs, table) if vs is not None else None
    first = None
    for max_len in (None, max(lens)):
        o = ops.attn_decode_paged(q, kp, vp, table, i32(lens), ks, vs, max_len=max_len)
        ref = ops.attn_decode_varlen(q, gk, gv, i32(lens), gks, gvs, max_len=max_len)
        diff = (o.float() - ref.float()).abs().max().item()
        print(f"{tag} max_len={max_len}: bit-equal to varlen on the gathered cache: "
              f"{torch.equal(o, ref)}, max abs diff {diff:.3e}")
        assert o.shape == q.shape and o.dtype == torch.bfloat16
        assert torch.equal(o, ref)
        first = o if first is None else first
    for b, t in enumerate(lens):
        if t == 0:
            assert (first[b] == 0).all(), first[b]
            continue
        want = decode_ref(q[b], kd[b, :t], vd[b, :t])
        print(f"{tag} b={b} t={t}: max abs err "
              f"{(first[b].float() - want).abs().max().item():.3e}")
        torch.testing.assert_close(first[b].float(), want, **TOL)
    # slots past a sequence's pages are never read: any value there, in range
    # or not, changes nothing
    for junk in (-1, n_pages + 5):
        t2 = table.clone()
        for b, t in enumerate(lens):
            t2[b, (t + PAGE - 1) // PAGE:] = junk
        o2 = ops.attn_decode_paged(q, kp, vp, t2, i32(lens), ks, vs)
        assert torch.equal(o2, first), junk
    assert max_pages * PAGE >= max(lens)


@pytest.mark.parametrize("shape", DECODE_SHAPES, ids=ids_of)
def test_decode_paged_kernel(shape):
    B, Hq, Hkv, D, max_pages, lens = shape
    T = max_pages * PAGE
    q = rand_bf16(B, Hq, D, seed=1)
    kc = rand_bf16(B, T, Hkv, D, seed=2)
    vc = rand_bf16(B, T, Hkv, D, seed=3)
    table, n_pages = make_table(lens, max_pages)
    kp = scatter_rows(kc, table, lens, n_pages)
    vp = scatter_rows(vc, table, lens, n_pages)
    _check_decode(ids_of(shape), q, (kp, vp), (None, None), table, n_pages, lens, kc, vc)


def _fp8_dense(B, T, Hkv, D, seed):
    cache = KVCache(B, T, Hkv, D, DEV, quant="fp8")
    cache.append(rand_bf16(B, T, Hkv, D, seed=seed), rand_bf16(B, T, Hkv, D, seed=seed + 1))
    return cache


def test_decode_paged_kernel_fp8():
    B, Hq, Hkv, D, max_pages, lens = DECODE_SHAPES[0]
    T = max_pages * PAGE
    q = rand_bf16(B, Hq, D, seed=4)
    cache = _fp8_dense(B, T, Hkv, D, 5)
    kd, vd = cache.dequant(T)  # quantisation error is common to both sides
    table, n_pages = make_table(lens, max_pages)
    pools = [scatter_rows(x, table, lens, n_pages)
             for x in (cache.k, cache.v, cache.k_scale, cache.v_scale)]
    assert pools[2].isnan().any() and (pools[0].view(torch.uint8) == 0x7F).any()
    _check_decode("fp8", q, pools[:2], pools[2:], table, n_pages, lens, kd, vd)


def test_decode_paged_aliased_pages():
    """Two sequences whose first two slots name the SAME pages (a shared
    prefix) give what two private copies of those pages give."""
    B, Hq, Hkv, D, max_pages = 2, 8, 2, 128, 3
    lens = [150, 140]
    q = rand_bf16(B, Hq, D, seed=7)
    kc = rand_bf16(B, max_pages * PAGE, Hkv, D, seed=8)
    vc = rand_bf16(B, max_pages * PAGE, Hkv, D, seed=9)
    kc[1, :2 * PAGE] = kc[0, :2 * PAGE]
    vc[1, :2 * PAGE] = vc[0, :2 * PAGE]
    private, n_pages = make_table(lens, max_pages)
    kp = scatter_rows(kc, private, lens, n_pages)
    vp = scatter_rows(vc, private, lens, n_pages)
    shared = private.clone()
    shared[1, :2] = private[0, :2]
    o_private = ops.attn_decode_paged(q, kp, vp, private, i32(lens))
    # the pages sequence 1 no longer names become poison
    for p in private[1, :2].tolist():
        kp[p] = float("nan")
        vp[p] = float("nan")
    o_shared = ops.attn_decode_paged(q, kp, vp, shared, i32(lens))
    assert torch.equal(o_shared, o_private) and not o_shared.isnan().any()


def test_paged_ops_argument_checks_gpu():
    B, Hq, Hkv, D, max_pages, lens = DECODE_SHAPES[1]
    q = rand_bf16(B, Hq, D, seed=1)
    table, n_pages = make_table(lens, max_pages)
    kp = rand_bf16(n_pages, PAGE, Hkv, D, seed=2)
    with pytest.raises(ValueError):
        ops.attn_decode_paged(q, kp, kp, table, i64(lens))
    with pytest.raises(ValueError):
        ops.attn_decode_paged(q, kp, kp, table, i32(lens), max_len=max_pages * PAGE + 1)
    with pytest.raises(ValueError):
        ops.attn_prefill_paged(q[:, None], kp, kp, table, max_pages * PAGE)
    with pytest.raises(ValueError):
        ops.kv_append_paged(kp[:B, :1], kp[:B, :1], kp, kp, table, i64([0, 0]))


# ---- prefill kernel -------------------------------------------------------

# (B, s, Hq, Hkv, D, pos, seq_lens)
PREFILL_SHAPES = [
    (2, 70, 4, 2, 64, 0, None),
    (2, 37, 8, 2, 128, 100, None),  # the chunk crosses a page boundary
    (3, 130, 4, 4, 64, 64, [194, 70, 64]),  # last sequence: no live row
]


def _check_prefill(tag, shape, q, pools, scales, table, kd, vd):
    B, s, Hq, Hkv, D, pos, seq_lens = shape
    kp, vp = pools
    ks, vs = scales
    lens_t = i32(seq_lens) if seq_lens is not None else None
    o = ops.attn_prefill_paged(q, kp, vp, table, pos, ks, vs, seq_lens=lens_t)
    gk, gv = gather_pages(kp, table), gather_pages(vp, table)
    gks = gather_pages(ks, table) if ks is not None else None
    gvs = gather_pages(vs, table) if vs is not None else None
    ref = ops.attn_prefill(q, gk, gv, pos, gks, gvs, seq_lens=lens_t)
    print(f"{tag}: bit-equal to attn_prefill on the gathered cache: "
          f"{torch.equal(o, ref)}, max abs diff "
          f"{(o.float() - ref.float()).abs().max().item():.3e}")
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    assert torch.equal(o, ref) and not o.isnan().any()
    t = pos + s
    if seq_lens is None:
        want = ops.reference.attention_cached(q, kd[:, :t], vd[:, :t], pos)
    else:
        want = _attention_cached_varlen(q, kd[:, :t], vd[:, :t], pos, lens_t)
        for b, n in enumerate(seq_lens):
            assert (o[b, max(0, n - pos):] == 0).all(), b
    print(f"{tag}: max abs err vs fp32 reference "
          f"{(o.float() - want.float()).abs().max().item():.3e}")
    torch.testing.assert_close(o.float(), want.float(), **TOL)


@pytest.mark.parametrize("shape", PREFILL_SHAPES, ids=ids_of)
def test_prefill_paged_kernel(shape):
    B, s, Hq, Hkv, D, pos, seq_lens = shape
    max_pages = (pos + s + PAGE - 1) // PAGE
    rows = seq_lens if seq_lens is not None else [pos + s] * B
    q = rand_bf16(B, s, Hq, D, seed=11)
    kc = rand_bf16(B, max_pages * PAGE, Hkv, D, seed=12)
    vc = rand_bf16(B, max_pages * PAGE, Hkv, D, seed=13)
    table, n_pages = make_table(rows, max_pages)
    kp = scatter_rows(kc, table, rows, n_pages)
    vp = scatter_rows(vc, table, rows, n_pages)
    _check_prefill(ids_of(shape), shape, q, (kp, vp), (None, None), table, kc, vc)


def test_prefill_paged_kernel_fp8():
    shape = PREFILL_SHAPES[2]
    B, s, Hq, Hkv, D, pos, seq_lens = shape
    max_pages = (pos + s + PAGE - 1) // PAGE
    q = rand_bf16(B, s, Hq, D, seed=14)
    cache = _fp8_dense(B, max_pages * PAGE, Hkv, D, 15)
    kd, vd = cache.dequant(max_pages * PAGE)
    table, n_pages = make_table(seq_lens, max_pages)
    pools = [scatter_rows(x, table, seq_lens, n_pages)
             for x in (cache.k, cache.v, cache.k_scale, cache.v_scale)]
    _check_prefill("fp8", shape, q, pools[:2], pools[2:], table, kd, vd)


# ---- append kernels -------------------------------------------------------


def _append_case(quant, D, k, v, table, n_pages, pos, lens):
    """Run ops.kv_append_paged on poisoned pools and compare every pool with
    what the row rule gives (computed row by row on the host's table)."""
    B, s, Hkv, _ = k.shape
    max_pages = table.shape[1]
    if quant:
        like = torch.empty(1, 1, Hkv, D, dtype=torch.float8_e4m3fn, device=DEV)
        names = ("k", "v", "k_scale", "v_scale")
        got = {"k": poisoned(n_pages, like), "v": poisoned(n_pages, like),
               "k_scale": poisoned(n_pages, torch.empty(1, 1, Hkv, device=DEV)),
               "v_scale": poisoned(n_pages, torch.empty(1, 1, Hkv, device=DEV))}
        kq, ksc = KVCache._quantize_rows(None, k)
        vq, vsc = KVCache._quantize_rows(None, v)
        src = {"k": kq, "v": vq, "k_scale": ksc, "v_scale": vsc}
    else:
        names = ("k", "v")
        got = {"k": poisoned(n_pages, k), "v": poisoned(n_pages, v)}
        src = {"k": k, "v": v}
    want = {n: got[n].clone() for n in names}
    host = table.cpu()
    pos_l = pos.tolist() if isinstance(pos, torch.Tensor) else [pos] * B
    if len(pos_l) == 1:
        pos_l = pos_l * B
    written = 0
    for b in range(B):
        for i in range(s):
            p = pos_l[b] + i
            if not 0 <= p < max_pages * PAGE or (lens is not None and p >= lens[b]):
                continue
            page = int(host[b, p // PAGE])
            if not 0 <= page < n_pages:
                continue
            written += 1
            for n in names:
                w, x = want[n], src[n]
                if w.dtype == torch.float8_e4m3fn:
                    w, x = w.view(torch.uint8), x.view(torch.uint8)
                w[page, p % PAGE] = x[b, i]
    ops.kv_append_paged(k, v, got["k"], got["v"], table, pos, got.get("k_scale"),
                        got.get("v_scale"), lens=None if lens is None else i32(lens))
    torch.cuda.synchronize()
    for n in names:
        assert same_bytes(got[n], want[n]), n
    return written


@pytest.mark.parametrize("quant", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("D", [64, 128])
def test_append_paged_single_rows(quant, D):
    B, Hkv, max_pages = 4, 2, 2
    k = rand_bf16(B, 1, Hkv, D, seed=21)
    v = rand_bf16(B, 1, Hkv, D, seed=22)
    table, n_pages = make_table([128] * B, max_pages)
    # the last sequence is parked: nothing of it is written anywhere
    pos = i64([5, 63, 64, max_pages * PAGE])
    assert _append_case(quant, D, k, v, table, n_pages, pos, None) == 3
    # a table entry of -1 (or past the pool) under a live position writes nothing
    t2 = table.clone()
    t2[0, 0] = -1
    t2[2, 1] = n_pages
    assert _append_case(quant, D, k, v, t2, n_pages, pos, None) == 1


@pytest.mark.parametrize("quant", [False, True], ids=["bf16", "fp8"])
def test_append_paged_chunk_with_lens(quant):
    B, s, Hkv, D, max_pages, pos = 4, 70, 2, 64, 2, 30
    lens = [100, 45, 30, 64]
    k = rand_bf16(B, s, Hkv, D, seed=23)
    v = rand_bf16(B, s, Hkv, D, seed=24)
    table, n_pages = make_table(lens, max_pages)
    assert _append_case(quant, D, k, v, table, n_pages, pos, lens) == 70 + 15 + 0 + 34
    # without lens every row with a page is written: the pads of sequence 1
    # up to the end of its only page, none on its -1 slot
    assert _append_case(quant, D, k, v, table, n_pages, i64([pos]), None) == 70 + 34 * 3


# ---- model ----------------------------------------------------------------


def _bf16_model(name, **kw):
    model = models.build(name, **kw).to(DEV).bfloat16().eval()
    for buf in model.buffers():  # rope tables stay fp32
        if buf.dtype is torch.bfloat16:
            buf.data = buf.data.float()
    return model


def _valid_agreement(tokens, lens, refs):
    eq = torch.cat([(tokens[b, :n] == refs[b][:n]).float()
                    for b, n in enumerate(lens)])
    return eq.mean().item()


@pytest.mark.parametrize("kw", [{}, {"kv_quant": "fp8"}, {"prefill_chunk": 48}],
                         ids=["bf16", "fp8", "chunk48"])
def test_generate_paged_equals_contiguous_ragged(monkeypatch, kw):
    """Eager paged against eager contiguous ragged: the only ops that differ
    are bit-equal, so the tokens are equal. Every pass is native (the
    reference attention is patched to raise)."""
    def boom(*a, **k):
        raise AssertionError("reference.attention_cached hit on the GPU path")

    monkeypatch.setattr(ops.reference, "attention_cached", boom)
    torch.manual_seed(17)
    model = _bf16_model("llama-tiny")
    lens, s, new = [200, 5, 70], 200, 8
    ids = torch.randint(0, 256, (3, s), device=DEV)
    pad = int(ids[0, 3])
    for b, n in enumerate(lens):
        ids[b, n:] = pad
    base = dict(max_new_tokens=new, prompt_lens=lens, pad_token_id=pad, **kw)
    want, want_lens = model.generate(ids, **base)
    got, got_lens = model.generate(ids, **base, kv_layout="paged",
                                   kv_free_order=scattered(7))
    agree = _valid_agreement(got, got_lens.tolist(), list(want))
    print(f"paged vs contiguous {kw}: equal {torch.equal(got, want)}, "
          f"agreement {agree:.3f}")
    assert got_lens.tolist() == want_lens.tolist() == [n + new for n in lens]
    assert torch.equal(got, want)
    with pytest.raises(PagePoolExhausted):
        model.generate(ids, **base, kv_layout="paged", kv_pages=6)


def test_graphed_decoder_paged():
    from hypha_amd.runtime.graphed_decode import GraphedDecoder

    torch.manual_seed(29)
    model = _bf16_model("llama-tiny", hidden_size=2048, n_heads=16, n_kv_heads=4,
                        ffn_hidden=4096, n_layers=2)
    lens, s, new, pad = [128, 70, 3, 97], 128, 24, 0
    ids = torch.randint(1, 500, (4, s), device=DEV)
    for b, n in enumerate(lens):
        ids[b, n:] = pad
    # pages of the batch: ceil((L_b + new) / 64) = 3 + 2 + 1 + 2
    dec = GraphedDecoder(model, batch=4, prompt_len=s, max_new=32, kv_layout="paged",
                         kv_pages=13, kv_free_order=scattered(13))
    eager, eager_lens = model.generate(ids, max_new_tokens=new, prompt_lens=lens,
                                       kv_layout="paged", kv_free_order=scattered(8))
    table_ptr = dec.table.table.data_ptr()
    graphed, g_lens = dec.generate(ids, max_new_tokens=new, prompt_lens=lens)
    assert dec.graph_r is not None  # really captured
    assert dec.graph is None and dec.graph_s is None
    assert dec.table.pages_in_use == 8
    assert graphed.shape == eager.shape == (4, s + new)
    assert g_lens.tolist() == eager_lens.tolist() == [n + new for n in lens]
    agree = _valid_agreement(graphed, g_lens.tolist(), list(eager))
    print(f"graphed paged vs eager paged: agreement {agree:.3f}")
    assert agree >= 0.97, (agree, graphed, eager)
    for b, n in enumerate(lens):
        assert (graphed[b, n + new:] == pad).all()

    # second call replays the captured graph over the refilled table
    graph_r = dec.graph_r
    graphed2, g_lens2 = dec.generate(ids, max_new_tokens=new, prompt_lens=lens)
    assert dec.graph_r is graph_r and dec.table.table.data_ptr() == table_ptr
    assert torch.equal(graphed2, graphed) and torch.equal(g_lens2, g_lens)

    # a uniform call goes through the same graph and returns tokens only
    full = torch.randint(1, 500, (4, s), device=DEV)
    uni = dec.generate(full, max_new_tokens=new)
    assert isinstance(uni, torch.Tensor) and uni.shape == (4, s + new)
    assert torch.equal(uni[:, :s], full) and dec.graph is None
    assert dec.table.pages_in_use == 12
    # ... and the ragged batch after it is served as before
    graphed3, _ = dec.generate(ids, max_new_tokens=new, prompt_lens=lens)
    assert torch.equal(graphed3, graphed)

    # sampled: the fourth graph, the same tokens for the same seed
    skw = dict(max_new_tokens=new, prompt_lens=lens, temperature=0.8, top_k=50,
               top_p=0.9, seed=5)
    s1, l1 = dec.generate(ids, **skw)
    assert dec.graph_rs is not None and dec.graph_s is None
    s2, l2 = dec.generate(ids, **skw)
    assert torch.equal(s1, s2) and torch.equal(l1, l2)

    # too few pages: refused before any step runs
    small = GraphedDecoder(model, batch=4, prompt_len=s, max_new=32, kv_layout="paged",
                           kv_pages=7)
    small.tokens_r.fill_(-7)
    with pytest.raises(PagePoolExhausted):
        small.generate(ids, max_new_tokens=new, prompt_lens=lens)
    assert (small.tokens_r == -7).all() and small.table.pages_in_use == 0
