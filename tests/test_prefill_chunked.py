"""Chunked / ragged prefill on the CPU reference path: ops.attn_prefill,
generate(prefill_chunk=...) on the three model families, and the inference
executor's "prefill_chunk" job key."""

import json
import math
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

REPO = Path(__file__).resolve().parent.parent
FAMILIES = ("llama-tiny", "moe-tiny", "gpt2-tiny")
PROMPT = 37


def naive_prefill(q, k, v, pos):
    """Row-by-row masked softmax, written independently of ops.reference:
    q [B,s,Hq,D]; k/v [B,t,Hkv,D]; q row i sees kv j <= pos + i."""
    B, s, Hq, D = q.shape
    G = Hq // k.shape[2]
    out = torch.zeros(B, s, Hq, D, dtype=torch.float64)
    for b in range(B):
        for h in range(Hq):
            for i in range(s):
                n = pos + i + 1
                kk = k[b, :n, h // G].double()
                vv = v[b, :n, h // G].double()
                w = torch.softmax(kk @ q[b, i, h].double() / math.sqrt(D), dim=0)
                out[b, i, h] = w @ vv
    return out


@pytest.mark.parametrize("pos,s,hq,hkv", [(0, 7, 4, 4), (5, 3, 4, 2), (9, 1, 6, 1)])
def test_attn_prefill_cpu_matches_naive(pos, s, hq, hkv):
    torch.manual_seed(pos + s)
    B, D, T_alloc = 2, 16, pos + s + 4
    q = torch.randn(B, s, hq, D)
    kc = torch.randn(B, T_alloc, hkv, D)
    vc = torch.randn(B, T_alloc, hkv, D)
    # rows past the valid length must not matter
    kc[:, pos + s:] = float("nan")
    vc[:, pos + s:] = float("nan")
    o = ops.attn_prefill(q, kc, vc, pos)
    assert o.shape == q.shape and o.dtype == q.dtype
    ref = naive_prefill(q, kc, vc, pos)
    torch.testing.assert_close(o.double(), ref, rtol=1e-5, atol=1e-5)


def test_attn_prefill_cpu_fp8_cache_uses_dequantized_rows():
    torch.manual_seed(3)
    B, s, H, D, pos = 1, 4, 2, 16, 6
    cache = KVCache(B, 12, H, D, "cpu", dtype=torch.float32, quant="fp8")
    cache.append(torch.randn(B, pos + s, H, D), torch.randn(B, pos + s, H, D))
    q = torch.randn(B, s, H, D)
    o = ops.attn_prefill(q, cache.k, cache.v, pos, cache.k_scale, cache.v_scale)
    kd, vd = cache.dequant(pos + s)
    ref = naive_prefill(q, kd.float(), vd.float(), pos)
    torch.testing.assert_close(o.double(), ref, rtol=1e-5, atol=1e-5)


def test_attn_prefill_rejects_overflowing_chunk():
    q = torch.randn(1, 4, 2, 16)
    kc = torch.randn(1, 8, 2, 16)
    with pytest.raises(ValueError):
        ops.attn_prefill(q, kc, kc, 5)  # 5 + 4 > 8


def _final_hidden(model, ids, chunk):
    """Last-position hidden state (after the final norm) of a prompt fed
    through the KV-cache path in pieces of at most `chunk` tokens."""
    cfg = model.cfg
    b, s = ids.shape
    is_gpt2 = hasattr(model, "wte")
    if is_gpt2:
        n_kv, hd = cfg.n_heads, cfg.hidden_size // cfg.n_heads
    else:
        n_kv, hd = cfg.n_kv_heads, cfg.head_dim
    caches = [KVCache(b, s, n_kv, hd, ids.device, dtype=torch.float32)
              for _ in model.blocks]
    with torch.no_grad():
        for p0 in range(0, s, chunk):
            piece = ids[:, p0:p0 + chunk]
            if is_gpt2:
                idx = torch.arange(p0, p0 + piece.shape[1])
                x = model.wte(piece) + model.wpe(idx)
                for blk, cache in zip(model.blocks, caches):
                    x = blk(x, cache=cache, pos=p0)
            else:
                x = model.embed(piece)
                for blk, cache in zip(model.blocks, caches):
                    x = blk(x, model.rope_cos, model.rope_sin, cache=cache, pos=p0)
                    x = x[0] if isinstance(x, tuple) else x  # MoE: (x, aux)
        norm = model.ln_f if is_gpt2 else model.norm
        return norm(x[:, -1:])


@pytest.fixture(scope="module")
def tiny_models():
    out = {}
    for name in FAMILIES:
        torch.manual_seed(11)
        model = models.build(name).float().eval()
        ids = torch.randint(0, 256, (2, PROMPT))
        out[name] = (model, ids, _final_hidden(model, ids, PROMPT))
    return out


@pytest.mark.parametrize("chunk", [16, 5, 1])
@pytest.mark.parametrize("name", FAMILIES)
def test_chunked_prefill_hidden_matches_one_shot(tiny_models, name, chunk):
    model, ids, one_shot = tiny_models[name]
    got = _final_hidden(model, ids, chunk)
    print(f"{name} chunk={chunk}: max abs diff "
          f"{(got - one_shot).abs().max().item():.3e}")
    torch.testing.assert_close(got, one_shot, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name", FAMILIES)
def test_generate_prefill_chunk_same_greedy_tokens(tiny_models, name):
    model, ids, _ = tiny_models[name]
    base = model.generate(ids, max_new_tokens=6)
    assert base.shape == (2, PROMPT + 6)
    for chunk in (16, 5, PROMPT, PROMPT + 10):
        out = model.generate(ids, max_new_tokens=6, prefill_chunk=chunk)
        assert torch.equal(out, base), (name, chunk)


@pytest.mark.parametrize("name", FAMILIES)
def test_generate_prefill_chunk_zero_raises(tiny_models, name):
    model, ids, _ = tiny_models[name]
    with pytest.raises(ValueError):
        model.generate(ids, max_new_tokens=2, prefill_chunk=0)


# ---------------------------------------------------------------------------
# inference executor: "prefill_chunk" job key
# ---------------------------------------------------------------------------


class UDSHttpServer(socketserver.ThreadingUnixStreamServer):
    daemon_threads = True


def _run_executor(tmp, slice_paths, extra):
    class Handler(BaseHTTPRequestHandler):
        def _json(self, obj):
            body = json.dumps(obj).encode()
            self.send_response(200)
            self.send_header("Content-Type", "application/json")
            self.send_header("Content-Length", str(len(body)))
            self.end_headers()
            self.wfile.write(body)

        def do_POST(self):
            n = int(self.headers.get("Content-Length", 0))
            self.rfile.read(n)
            if self.path == "/resources/fetch":
                self._json({"files": slice_paths})
            else:
                self._json({"kind": "ok"})

        def log_message(self, *a):
            pass

    tmp.mkdir()
    sock_path = str(tmp / "bridge.sock")
    server = UDSHttpServer(sock_path, Handler)
    threading.Thread(target=server.serve_forever, daemon=True).start()
    work = tmp / "work"
    work.mkdir()
    job = tmp / "job.json"
    cfg = {"model": "llama-tiny", "data": {"any": "ref"}, "batch_size": 2,
           "seq_len": 16, "max_new_tokens": 4, "num_batches": 1, "seed": 0}
    cfg.update(extra)
    job.write_text(json.dumps(cfg))
    try:
        r = subprocess.run(
            [sys.executable, "-m", "hypha_amd.runtime.infer_executor",
             "--socket", sock_path, "--work-dir", str(work), "--job", str(job)],
            cwd=REPO,
            # the executor runs on the CPU here, so its tokens can be compared
            # with an in-process fp32 model on any machine
            env=dict(os.environ, PYTHONPATH=str(REPO), HIP_VISIBLE_DEVICES="",
                     CUDA_VISIBLE_DEVICES=""),
            capture_output=True, text=True, timeout=180,
        )
    finally:
        server.shutdown()
        server.server_close()
    return r, work


def test_infer_executor_honours_prefill_chunk(short_tmp_path):
    from safetensors.torch import load_file

    from hypha_amd.data.synthetic import load_slice, write_slice_files

    slice_paths = write_slice_files(str(short_tmp_path / "slices"), "p", 1, 4, 512, 32)

    # a chunk size the job would reject proves the key is read ...
    r, _ = _run_executor(short_tmp_path / "bad", slice_paths, {"prefill_chunk": 0})
    assert r.returncode != 0
    assert "prefill_chunk" in r.stderr

    # ... and a valid one yields the tokens of a direct chunked generate()
    r, work = _run_executor(short_tmp_path / "ok", slice_paths, {"prefill_chunk": 5})
    assert r.returncode == 0, r.stderr[-2000:]
    outs = sorted(work.glob("completion-*.safetensors"))
    assert len(outs) == 1
    tokens = load_file(str(outs[0]))["tokens"]
    assert tokens.shape == (2, 20)

    torch.manual_seed(0)  # the executor seeds from the job's "seed"
    model = models.build("llama-tiny").float().eval()
    prompts = load_slice(slice_paths[0])[:2, :16]
    expect = model.generate(prompts, max_new_tokens=4, prefill_chunk=5)
    assert torch.equal(tokens, expect)
