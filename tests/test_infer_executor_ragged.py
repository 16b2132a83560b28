"""Inference executor with "pad_token_id" / "eos_token_id": prompt lengths are
taken from the right-padded rows, the batch is generated ragged, and the
completion file carries "lens" next to "tokens"."""

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

REPO = Path(__file__).resolve().parent.parent


class UDSHttpServer(socketserver.ThreadingUnixStreamServer):
    daemon_threads = True


@pytest.fixture
def tmp_path(short_tmp_path):
    # bridge.sock is bound inside it: a Unix socket path holds < 108 bytes
    return short_tmp_path


def test_prompt_lengths_strip_only_the_trailing_pad_run():
    from hypha_amd.runtime.infer_executor import prompt_lengths

    pad = 7
    rows = torch.tensor([[1, 2, 3, 4, 5, 6],     # no pad
                         [1, 7, 3, 7, 7, 7],     # pad id inside the prompt stays
                         [7, 7, 7, 7, 7, 7],     # all pad: one token is kept
                         [7, 7, 2, 7, 7, 7]])
    assert prompt_lengths(rows, pad).tolist() == [6, 3, 1, 3]


def test_infer_executor_ragged_end_to_end(tmp_path):
    from safetensors.torch import load_file, save_file

    from hypha_amd import models

    pad, seq_len, new = 3, 12, 4
    lens = [12, 5]
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(4, 512, (2, seq_len), generator=g)
    for b, n in enumerate(lens):
        ids[b, n:] = pad
    slice_dir = tmp_path / "slices"
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

    sock_path = str(tmp_path / "bridge.sock")
    server = UDSHttpServer(sock_path, Handler)
    threading.Thread(target=server.serve_forever, daemon=True).start()
    work = tmp_path / "work"
    work.mkdir()
    job = tmp_path / "job.json"
    job.write_text(json.dumps({
        "model": "llama-tiny", "data": {"any": "ref"}, "seed": 0,
        "batch_size": 2, "seq_len": seq_len, "max_new_tokens": new, "num_batches": 1,
        "pad_token_id": pad,
    }))
    r = subprocess.run(
        [sys.executable, "-m", "hypha_amd.runtime.infer_executor",
         "--socket", sock_path, "--work-dir", str(work), "--job", str(job)],
        cwd=REPO, env=dict(os.environ, PYTHONPATH=str(REPO)),
        capture_output=True, text=True, timeout=180,
    )
    server.shutdown()
    assert r.returncode == 0, r.stderr[-2000:]
    out = load_file(str(work / "completion-00000.safetensors"))
    assert out["tokens"].shape == (2, seq_len + new)
    assert out["lens"].tolist() == [n + new for n in lens]
    for b, n in enumerate(lens):
        assert torch.equal(out["tokens"][b, :n], ids[b, :n])
        assert (out["tokens"][b, n + new:] == pad).all()
    if not torch.cuda.is_available():
        # the executor seeds the same fp32 model on the CPU: the short prompt
        # continues exactly as it does on its own
        torch.manual_seed(0)
        model = models.build("llama-tiny").eval()
        alone = model.generate(ids[1:2, :5], max_new_tokens=new, seed=0)[0]
        assert torch.equal(out["tokens"][1, :5 + new], alone)
