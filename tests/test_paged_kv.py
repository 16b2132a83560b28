"""Paged KV cache on the CPU: the page table, the reference paths of the three
paged ops against the contiguous reference on the gathered cache, the paged
route of llama generate against the contiguous ragged route, and the
inference executor's "kv_layout" key."""

import json
import os
import socketserver
import subprocess
import sys
import threading
from http.server import BaseHTTPRequestHandler
from pathlib import Path

import pytest
import torch

from hypha_amd import models, ops
from hypha_amd.models.kv_cache import KVCache
from hypha_amd.models.paged_kv import (PAGE, PagedKVCache, PagePoolExhausted,
                                       PageTable)

REPO = Path(__file__).resolve().parent.parent


def scattered(n):
    """A permutation of range(n) with no two neighbours adjacent pages (n odd
    or even): evens descending, then odds ascending."""
    return [p for p in range(n - 1, -1, -1) if p % 2 == 0] + \
           [p for p in range(n) if p % 2 == 1]


# ---- PageTable --------------------------------------------------------------


def test_page_table_reserve_hands_out_pages_in_free_order():
    order = scattered(9)
    t = PageTable(3, 4, 9, "cpu", free_order=order)
    assert t.pages_in_use == 0 and (t.table == -1).all()
    ptr = t.table.data_ptr()
    t.reserve([208, 13, 78])  # 4, 1, 2 pages
    assert t.pages_in_use == 7
    assert t.table.dtype == torch.int32 and t.table.shape == (3, 4)
    assert t.table[0].tolist() == order[:4]
    assert t.table[1].tolist() == order[4:5] + [-1] * 3
    assert t.table[2].tolist() == order[5:7] + [-1] * 2
    assert torch.equal(t.table, t.host)
    # a second reservation frees everything first and reuses the pool
    t.reserve([64, 65, 1])  # 1, 2, 1 pages
    assert t.pages_in_use == 4
    assert t.table[0].tolist() == order[:1] + [-1] * 3
    assert t.table[1].tolist() == order[1:3] + [-1] * 2
    assert t.table[2].tolist() == order[3:4] + [-1] * 3
    assert t.table.data_ptr() == ptr  # rewritten in place
    t.reserve([0, 0, 0])
    assert t.pages_in_use == 0 and (t.table == -1).all()


def test_page_table_pool_exhausted_changes_nothing():
    PageTable(3, 4, 7, "cpu").reserve([208, 13, 78])
    ok = PageTable(3, 4, 7, "cpu", free_order=scattered(7))
    ok.reserve([208, 13, 78])
    assert ok.pages_in_use == 7
    t = PageTable(3, 4, 6, "cpu", free_order=scattered(6))
    t.reserve([64, 64, 64])
    before, used = t.table.clone(), t.pages_in_use
    with pytest.raises(PagePoolExhausted):
        t.reserve([208, 13, 78])
    assert issubclass(PagePoolExhausted, RuntimeError)
    assert torch.equal(t.table, before) and torch.equal(t.host, before)
    assert t.pages_in_use == used
    with pytest.raises(ValueError):
        t.reserve([257, 1, 1])  # 5 pages: more than the table has slots
    with pytest.raises(ValueError):
        t.reserve([1, 1])
    with pytest.raises(ValueError):
        PageTable(3, 4, 6, "cpu", free_order=[0, 1, 2, 3, 4, 4])


# ---- reference paths of the ops ---------------------------------------------

B, HQ, HKV, D, MAXP, NP = 3, 4, 2, 16, 4, 12
LENS = [200, 5, 70]


def _table(lens=LENS):
    t = PageTable(B, MAXP, NP, "cpu", free_order=scattered(NP))
    t.reserve(lens)
    return t


def _rand(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _filled(quant, lens=LENS):
    """A paged cache and a contiguous one holding the same rows: sequence b
    has lens[b] rows; every other pool row is poisoned."""
    table = _table(lens)
    dtype = torch.float32
    paged = PagedKVCache(table, HKV, D, "cpu", dtype=dtype, quant=quant)
    if quant == "fp8":
        paged.k.view(torch.uint8).fill_(0x7F)
        paged.v.view(torch.uint8).fill_(0x7F)
        paged.k_scale.fill_(float("nan"))
        paged.v_scale.fill_(float("nan"))
    else:
        paged.k.fill_(float("nan"))
        paged.v.fill_(float("nan"))
    T = MAXP * PAGE
    dense = KVCache(B, T, HKV, D, "cpu", dtype=dtype, quant=quant)
    k, v = _rand(B, T, HKV, D, seed=1), _rand(B, T, HKV, D, seed=2)
    dense.append(k, v)
    paged.append_chunk(k, v, 0, torch.tensor(lens, dtype=torch.int32))
    return paged, dense, k, v


@pytest.mark.parametrize("quant", [None, "fp8"], ids=["fp32", "fp8"])
def test_append_reference_writes_only_owned_rows(quant):
    paged, dense, k, v = _filled(quant)
    gk, gv, gks, gvs = paged.gather()
    for b, n in enumerate(LENS):
        if quant == "fp8":
            assert torch.equal(gk[b, :n].view(torch.uint8), dense.k[b, :n].view(torch.uint8))
            assert torch.equal(gv[b, :n].view(torch.uint8), dense.v[b, :n].view(torch.uint8))
            assert torch.equal(gks[b, :n], dense.k_scale[b, :n])
            assert torch.equal(gvs[b, :n], dense.v_scale[b, :n])
        else:
            assert torch.equal(gk[b, :n], k[b, :n]) and torch.equal(gv[b, :n], v[b, :n])
    # everything no sequence owns is still poison
    owned = torch.zeros(NP, PAGE, dtype=torch.bool)
    for b, n in enumerate(LENS):
        for j in range(n):
            owned[paged.table.host[b, j // PAGE], j % PAGE] = True
    if quant == "fp8":
        assert (paged.k.view(torch.uint8)[~owned] == 0x7F).all()
        assert paged.v_scale[~owned].isnan().all()
    else:
        assert paged.k[~owned].isnan().all() and paged.v[~owned].isnan().all()
        assert not paged.k[owned].isnan().any()


def _same_bytes(a, b):
    """Equal bit for bit (NaN poison included)."""
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("quant", [None, "fp8"], ids=["fp32", "fp8"])
def test_append_rows_reference_parks_and_skips_bad_pages(quant):
    paged, _, _, _ = _filled(quant, [5, 63, 64])
    host = paged.table.host
    k1, v1 = _rand(B, 1, HKV, D, seed=3), _rand(B, 1, HKV, D, seed=4)
    # sequence 2 owns one page and sits at position 64: its slot 1 is -1, so
    # nothing is written for it
    pos = torch.tensor([5, 63, 64])
    assert host[2, 1] == -1
    want = {n: getattr(paged, n).clone() for n in ("k", "v")}
    if quant:
        want.update({n: getattr(paged, n).clone() for n in ("k_scale", "v_scale")})
    for b in (0, 1):
        page, r = int(host[b, 0]), int(pos[b])
        for n, x in (("k", k1), ("v", v1)):
            if quant:
                q, sc = KVCache._quantize_rows(None, x[b, 0])
                want[n].view(torch.uint8)[page, r] = q.view(torch.uint8)
                want[n + "_scale"][page, r] = sc
            else:
                want[n][page, r] = x[b, 0]
    paged.append_rows(k1, v1, pos)
    for n, w in want.items():
        assert _same_bytes(getattr(paged, n), w), n
    # parked: nothing is written anywhere
    paged.append_rows(k1, v1, torch.full((B,), paged.table.max_rows))
    paged.append_rows(k1, v1, torch.full((B,), -1))
    for n, w in want.items():
        assert _same_bytes(getattr(paged, n), w), n


@pytest.mark.parametrize("quant", [None, "fp8"], ids=["fp32", "fp8"])
def test_decode_reference_equals_contiguous_on_gathered_cache(quant):
    paged, dense, _, _ = _filled(quant)
    q = _rand(B, HQ, D, seed=5)
    lens = torch.tensor(LENS[:2] + [0], dtype=torch.int32)
    gk, gv, gks, gvs = paged.gather()
    for max_len in (None, 200):
        o = ops.attn_decode_paged(q, paged.k, paged.v, paged.table.table, lens,
                                  paged.k_scale, paged.v_scale, max_len=max_len)
        ref = ops.attn_decode_varlen(q, gk, gv, lens, gks, gvs, max_len=max_len)
        assert torch.equal(o, ref) and not o.isnan().any()
        dense_o = ops.attn_decode_varlen(q, dense.k, dense.v, lens, dense.k_scale,
                                         dense.v_scale, max_len=max_len)
        assert torch.equal(o, dense_o)
        assert (o[2] == 0).all()


@pytest.mark.parametrize("quant", [None, "fp8"], ids=["fp32", "fp8"])
@pytest.mark.parametrize("with_lens", [False, True], ids=["full", "seq_lens"])
def test_prefill_reference_equals_contiguous_on_gathered_cache(quant, with_lens):
    lens = LENS if with_lens else [200, 200, 200]
    paged, dense, _, _ = _filled(quant, lens)
    pos, s = 60, 140  # crosses two page boundaries; pos + s = 200
    q = _rand(B, s, HQ, D, seed=6)
    seq_lens = torch.tensor(lens, dtype=torch.int32) if with_lens else None
    gk, gv, gks, gvs = paged.gather()
    o = ops.attn_prefill_paged(q, paged.k, paged.v, paged.table.table, pos,
                               paged.k_scale, paged.v_scale, seq_lens=seq_lens)
    ref = ops.attn_prefill(q, gk, gv, pos, gks, gvs, seq_lens=seq_lens)
    assert torch.equal(o, ref) and not o.isnan().any()
    dense_o = ops.attn_prefill(q, dense.k, dense.v, pos, dense.k_scale, dense.v_scale,
                               seq_lens=seq_lens)
    assert torch.equal(o, dense_o)
    if with_lens:
        assert (o[1] == 0).all()  # 5 rows: no live q row in this chunk
        assert (o[2, 10:] == 0).all()


def test_paged_ops_argument_checks():
    paged, _, _, _ = _filled(None)
    t = paged.table.table
    q = _rand(B, HQ, D, seed=7)
    lens = torch.tensor(LENS, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.attn_decode_paged(q, paged.k, paged.v, t, lens.long())
    with pytest.raises(ValueError):
        ops.attn_decode_paged(q, paged.k, paged.v, t.long(), lens)
    with pytest.raises(ValueError):
        ops.attn_decode_paged(q, paged.k, paged.v, t, lens, max_len=MAXP * PAGE + 1)
    with pytest.raises(ValueError):
        ops.attn_decode_paged(q, paged.k[:, :32], paged.v[:, :32], t, lens)
    with pytest.raises(ValueError):  # fp8 pool without scales
        ops.attn_decode_paged(q, paged.k.to(torch.float8_e4m3fn),
                              paged.v.to(torch.float8_e4m3fn), t, lens)
    q4 = _rand(B, 8, HQ, D, seed=8)
    with pytest.raises(ValueError):
        ops.attn_prefill_paged(q4, paged.k, paged.v, t, MAXP * PAGE - 7)
    with pytest.raises(ValueError):
        ops.attn_prefill_paged(q4, paged.k, paged.v, t[:2], 0)
    k = _rand(B, 2, HKV, D, seed=9)
    with pytest.raises(ValueError):
        ops.kv_append_paged(k, k, paged.k, paged.v, t, torch.zeros(2, dtype=torch.long))
    with pytest.raises(ValueError):
        ops.kv_append_paged(k, k, paged.k, paged.v, t, torch.zeros(B, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.kv_append_paged(k[..., :8], k[..., :8], paged.k, paged.v, t, 0)


# ---- model ------------------------------------------------------------------


def _pick_stop(tokens, lens, new, pad):
    """As tests/test_gpu_ragged.py: (b, step, id), a token sequence b first
    emits at a step that is neither the first nor the last, and that some
    other sequence never emits."""
    gen = [tokens[b, n:n + new].tolist() for b, n in enumerate(lens)]
    for b, toks in enumerate(gen):
        for step in range(1, new - 1):
            e = toks[step]
            if e == pad or e in toks[:step]:
                continue
            if any(e not in other for o, other in enumerate(gen) if o != b):
                return b, step, e
    raise AssertionError(f"no usable stop token in {gen}")


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(17)
    model = models.build("llama-tiny").eval()
    lens, s, new = [200, 5, 70], 200, 8
    ids = torch.randint(0, 256, (3, s))
    pad = int(ids[0, 3])
    for b, n in enumerate(lens):
        ids[b, n:] = pad
    base = dict(max_new_tokens=new, prompt_lens=lens, pad_token_id=pad)
    ref = model.generate(ids, **base)
    return model, ids, lens, new, pad, base, ref


PAGED = dict(kv_layout="paged", kv_free_order=scattered(7))


@pytest.mark.parametrize("kw", [{}, {"kv_quant": "fp8"}, {"prefill_chunk": 48}],
                         ids=["fp32", "fp8", "chunk48"])
def test_generate_paged_equals_contiguous_ragged(tiny, kw):
    model, ids, lens, new, pad, base, ref = tiny
    want = ref if not kw else model.generate(ids, **base, **kw)
    tokens, out_lens = model.generate(ids, **base, **kw, **PAGED)
    assert out_lens.tolist() == [n + new for n in lens]
    assert torch.equal(tokens, want[0]) and torch.equal(out_lens, want[1])


def test_generate_paged_stop_token(tiny):
    model, ids, lens, new, pad, base, ref = tiny
    _, _, eos = _pick_stop(ref[0], lens, new, pad)
    want = model.generate(ids, **base, eos_token_id=eos)
    got = model.generate(ids, **base, eos_token_id=eos, **PAGED)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert want[1].tolist() != ref[1].tolist()  # the stop really cut a sequence


def test_generate_paged_uniform_prompts_return_tokens_only(tiny):
    model, ids, _, new, _, _, _ = tiny
    b, s = 3, 70
    prompts = ids[:, :s].clone()
    prompts[1] = ids[0, 100:100 + s]  # no pads: three full prompts
    want = model.generate(prompts, max_new_tokens=new, prompt_lens=[s] * b)[0]
    got = model.generate(prompts, max_new_tokens=new, kv_layout="paged",
                         kv_free_order=scattered(6))
    assert isinstance(got, torch.Tensor) and torch.equal(got, want)
    sampled = dict(max_new_tokens=new, temperature=0.8, top_k=20, seed=3)
    for extra in ({}, {"sampler": "philox", "top_p": 0.9}):
        want = model.generate(prompts, prompt_lens=[s] * b, **sampled, **extra)[0]
        got = model.generate(prompts, kv_layout="paged", **sampled, **extra)
        assert torch.equal(got, want)


def test_generate_paged_pool_too_small(tiny):
    model, ids, _, _, _, base, _ = tiny
    with pytest.raises(PagePoolExhausted):  # 4 + 1 + 2 = 7 pages needed
        model.generate(ids, **base, kv_layout="paged", kv_pages=6)
    model.generate(ids, **base, kv_layout="paged", kv_pages=7)
    with pytest.raises(ValueError):
        model.generate(ids, **base, kv_layout="bogus")


# ---- inference executor -----------------------------------------------------


class UDSHttpServer(socketserver.ThreadingUnixStreamServer):
    daemon_threads = True


@pytest.fixture
def tmp_path(short_tmp_path):
    # bridge.sock is bound inside it: a Unix socket path holds < 108 bytes
    return short_tmp_path


def _run_job(tmp_path, name, ids, extra):
    from safetensors.torch import load_file, save_file

    slice_dir = tmp_path / f"slices-{name}"
    slice_dir.mkdir()
    slice_path = str(slice_dir / "p-00000.safetensors")
    save_file({"input_ids": ids}, slice_path)

    class Handler(BaseHTTPRequestHandler):
        def do_POST(self):
            n = int(self.headers.get("Content-Length", 0))
            self.rfile.read(n)
            obj = {"files": [slice_path]} if self.path == "/resources/fetch" else {"kind": "ok"}
            body = json.dumps(obj).encode()
            self.send_response(200)
            self.send_header("Content-Type", "application/json")
            self.send_header("Content-Length", str(len(body)))
            self.end_headers()
            self.wfile.write(body)

        def log_message(self, *a):
            pass

    sock_path = str(tmp_path / f"{name}.sock")
    server = UDSHttpServer(sock_path, Handler)
    threading.Thread(target=server.serve_forever, daemon=True).start()
    work = tmp_path / f"work-{name}"
    work.mkdir()
    job = tmp_path / f"job-{name}.json"
    job.write_text(json.dumps({
        "model": "llama-tiny", "data": {"any": "ref"}, "seed": 0,
        "batch_size": ids.shape[0], "seq_len": ids.shape[1], "max_new_tokens": 4,
        "num_batches": 1, "pad_token_id": 3, **extra,
    }))
    r = subprocess.run(
        [sys.executable, "-m", "hypha_amd.runtime.infer_executor",
         "--socket", sock_path, "--work-dir", str(work), "--job", str(job)],
        cwd=REPO, env=dict(os.environ, PYTHONPATH=str(REPO)),
        capture_output=True, text=True, timeout=180,
    )
    server.shutdown()
    server.server_close()
    out = work / "completion-00000.safetensors"
    return r, (load_file(str(out)) if out.exists() else None)


def test_infer_executor_paged_layout(tmp_path):
    pad, seq_len = 3, 70
    lens = [70, 5]
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(4, 512, (2, seq_len), generator=g)
    for b, n in enumerate(lens):
        ids[b, n:] = pad
    r0, dense = _run_job(tmp_path, "dense", ids, {})
    assert r0.returncode == 0, r0.stderr[-2000:]
    r1, paged = _run_job(tmp_path, "paged", ids, {"kv_layout": "paged", "kv_pages": 3})
    assert r1.returncode == 0, r1.stderr[-2000:]
    assert paged["tokens"].shape == (2, seq_len + 4)
    assert paged["lens"].tolist() == [n + 4 for n in lens]
    if not torch.cuda.is_available():  # the same fp32 model on the CPU: exact
        assert torch.equal(paged["tokens"], dense["tokens"])
        assert torch.equal(paged["lens"], dense["lens"])
    else:  # graphed bf16 decoders: the ragged tests' pooled bar
        eq = torch.cat([(paged["tokens"][b, :n + 4] == dense["tokens"][b, :n + 4]).float()
                        for b, n in enumerate(lens)])
        assert eq.mean().item() >= 0.97
    r2, none = _run_job(tmp_path, "bogus", ids, {"kv_layout": "bogus"})
    assert r2.returncode != 0 and none is None
    assert "kv_layout" in r2.stderr
