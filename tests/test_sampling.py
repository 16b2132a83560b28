"""Token sampling contract on the CPU: Philox4x32-10 known answers, the
sample_token reference against an independent brute-force implementation,
model.generate(sampler="philox"), and the executor's "sampler" job key."""

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
from hypha_amd.ops import reference

REPO = Path(__file__).resolve().parent.parent
NEG_INF = float("-inf")


# ---------------------------------------------------------------------------
# Philox
# ---------------------------------------------------------------------------

def _philox_py(counter, key):
    """Plain-int Philox4x32-10 (independent of the tensor implementation)."""
    c, k = list(counter), list(key)
    for r in range(10):
        if r:
            k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF,
             (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
    return c


KNOWN = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    got = reference.philox4x32(torch.tensor([counter]), torch.tensor([key]))[0].tolist()
    assert " ".join(f"{x:08x}" for x in got) == want
    assert _philox_py(counter, key) == got


def test_philox_uniform_seed_1234():
    x0 = {(0, 0): 0x2090B348, (0, 1): 0x9EEEDE35, (1, 0): 0x70C51B59, (1, 1): 0x81327A55}
    for step in (0, 1):
        u = ops.philox_uniform(1234, step, 2)
        assert u.dtype == torch.float32 and u.shape == (2,)
        for row in (0, 1):
            assert u[row].item() == (x0[(step, row)] >> 8) * 2.0 ** -24
    assert ops.philox_uniform(1234, 0, 1).item() == 0.1272079348564148


@pytest.mark.parametrize("seed,step", [(2 ** 32 + 5, 3), (7, 2 ** 32 + 9),
                                       (2 ** 62 + 12345, 2 ** 40 + 1), (0, 0)])
def test_philox_uniform_wide_seed_and_step(seed, step):
    u = ops.philox_uniform(seed, step, 5)
    ut = ops.philox_uniform(torch.tensor([seed]), torch.tensor([step]), 5)
    for row in range(5):
        x = _philox_py((row, step & 0xFFFFFFFF, step >> 32, 0),
                       (seed & 0xFFFFFFFF, seed >> 32))[0]
        assert u[row].item() == (x >> 8) * 2.0 ** -24
    assert torch.equal(u, ut)
    assert (u >= 0).all() and (u < 1).all()
    if seed >= 2 ** 32 or step >= 2 ** 32:  # the high words matter
        low = ops.philox_uniform(seed & 0xFFFFFFFF, step & 0xFFFFFFFF, 5)
        assert not torch.equal(u, low)


# ---------------------------------------------------------------------------
# sample_token: reference against brute force
# ---------------------------------------------------------------------------

def brute_force(row, u, t, k=0, p=1.0):
    """The contract, token by token, in Python floats."""
    v = len(row)
    vals = [0.0 if x == 0 else float(x) for x in row]  # -0.0 == +0.0
    order = sorted(range(v), key=lambda i: (-vals[i], i))
    zmax = vals[order[0]]
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)  # noqa: E731
    mass = [0.0 if vals[i] == NEG_INF else
            float(torch.exp((f32(vals[i]) - f32(zmax)) / f32(t))) for i in order]
    n = k if 0 < k < v else v
    zk = math.fsum(mass[:n])
    if p < 1:
        cum = 0.0
        for j in range(n):
            cum = math.fsum(mass[:j + 1])
            if cum >= p * zk:
                n = j + 1
                break
    zkept = math.fsum(mass[:n])
    for j in range(n):
        if math.fsum(mass[:j + 1]) > u * zkept:
            return order[j]
    return order[max(j for j in range(n) if mass[j] > 0)]


@pytest.mark.parametrize("t,k,p", [(1.0, 0, 1.0), (0.7, 5, 1.0), (1.3, 0, 0.9),
                                   (0.8, 12, 0.95), (0.5, 100, 0.5)])
def test_reference_matches_brute_force(t, k, p):
    g = torch.Generator().manual_seed(11)
    logits = (torch.randn(6, 40, generator=g) * 3).bfloat16().float()  # ties appear
    logits[1, 7] = NEG_INF
    logits[2, 3] = -0.0
    logits[2, 9] = 0.0
    for u in (0.0, 0.013, 0.31, 0.5, 0.77, 0.97, 1 - 2.0 ** -24):
        uu = torch.full((6,), u)
        got = ops.sample_token(logits, uu, t, k, p)
        assert got.shape == (6, 1) and got.dtype == torch.long
        want = [brute_force(logits[b].tolist(), float(uu[b]), t, k, p) for b in range(6)]
        assert got[:, 0].tolist() == want, (u, got[:, 0].tolist(), want)


def test_all_equal_row_inverts_the_uniform():
    v = 1000
    logits = torch.full((1, v), 1.5)
    for j in list(range(0, v, 37)) + [v - 1]:
        assert ops.sample_token(logits, torch.tensor([(j + 0.5) / v]), 1.0).item() == j


def test_one_dominant_logit_wins_for_every_u():
    logits = torch.zeros(1, 300)
    logits[0, 123] = 30.0
    for u in (0.0, 0.25, 0.5, 0.999, 1 - 2.0 ** -24):
        assert ops.sample_token(logits, torch.tensor([u]), 1.0).item() == 123


def test_top_k_1_is_the_lowest_index_argmax():
    logits = torch.zeros(2, 50)
    logits[0, [17, 4, 33]] = 2.0
    logits[1, [49, 48]] = 1.0
    for u in (0.0, 0.5, 0.99):
        got = ops.sample_token(logits, torch.tensor([u, u]), 0.8, top_k=1)
        assert got[:, 0].tolist() == [4, 48]


def test_top_k_at_least_v_is_off():
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(4, 64, generator=g)
    u = torch.rand(4, generator=g)
    off = ops.sample_token(logits, u, 0.9, top_k=0)
    assert torch.equal(ops.sample_token(logits, u, 0.9, top_k=64), off)
    assert torch.equal(ops.sample_token(logits, u, 0.9, top_k=10 ** 6), off)


def test_tiny_top_p_keeps_only_the_first_token():
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(4, 64, generator=g)
    logits[3, [5, 9]] = 9.0  # tied maxima: the lower index
    for u in (0.0, 0.6, 0.999):
        got = ops.sample_token(logits, torch.full((4,), u), 1.0, top_p=1e-6)
        want = logits.argmax(-1).tolist()[:3] + [5]
        assert got[:, 0].tolist() == want


def test_minus_inf_is_never_returned():
    logits = torch.full((1, 16), NEG_INF)
    logits[0, [2, 11]] = 0.0
    seen = {ops.sample_token(logits, torch.tensor([u]), 1.0).item()
            for u in (0.0, 0.1, 0.49, 0.51, 0.9, 1 - 2.0 ** -24)}
    assert seen == {2, 11}


def test_signed_zeros_tie_by_index():
    logits = torch.full((1, 8), -5.0)
    logits[0, 2] = -0.0
    logits[0, 5] = 0.0
    assert ops.sample_token(logits, torch.tensor([0.0]), 1.0, top_k=1).item() == 2
    logits[0, 2], logits[0, 5] = 0.0, -0.0
    assert ops.sample_token(logits, torch.tensor([0.0]), 1.0, top_k=1).item() == 2
    assert ops.sample_token(logits, torch.tensor([0.75]), 1.0, top_k=2).item() == 5


def test_tensor_parameters_agree_with_numbers():
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(3, 100, generator=g)
    u = torch.rand(3, generator=g)
    a = ops.sample_token(logits, u, 0.8, 20, 0.9)
    b = ops.sample_token(logits, u, torch.tensor([0.8]), torch.tensor([20]),
                         torch.tensor([0.9]))
    assert torch.equal(a, b)


def test_nan_row_stays_in_range():
    logits = torch.randn(2, 33)
    logits[0, 4] = float("nan")
    logits[1, :] = float("nan")
    got = ops.sample_token(logits, torch.tensor([0.3, 0.7]), 1.0, 5, 0.9)
    assert ((got >= 0) & (got < 33)).all()


@pytest.mark.parametrize("kw", [dict(temperature=0.0), dict(temperature=-1.0),
                                dict(temperature=1.0, top_p=0.0),
                                dict(temperature=1.0, top_p=1.5),
                                dict(temperature=1.0, top_k=-1)])
def test_sample_token_value_errors(kw):
    with pytest.raises(ValueError):
        ops.sample_token(torch.zeros(1, 8), torch.zeros(1), **kw)


# ---------------------------------------------------------------------------
# model.generate(sampler="philox")
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(0)
    return models.build("llama-tiny").eval()


@pytest.fixture(scope="module")
def prompt():
    return torch.randint(4, 512, (2, 9), generator=torch.Generator().manual_seed(2))


SAMPLE = dict(temperature=0.8, top_k=20, top_p=0.9, sampler="philox")


def test_generate_philox_is_a_function_of_the_seed(tiny, prompt):
    a = tiny.generate(prompt, max_new_tokens=6, seed=3, **SAMPLE)
    assert a.shape == (2, 15) and torch.equal(a[:, :9], prompt)
    assert torch.equal(a, tiny.generate(prompt, max_new_tokens=6, seed=3, **SAMPLE))
    assert not torch.equal(a, tiny.generate(prompt, max_new_tokens=6, seed=4, **SAMPLE))


def test_generate_philox_top_k_1_is_greedy(tiny, prompt):
    greedy = tiny.generate(prompt, max_new_tokens=6)
    got = tiny.generate(prompt, max_new_tokens=6, temperature=0.8, top_k=1, seed=3,
                        sampler="philox")
    assert torch.equal(got, greedy)


def test_generate_philox_ragged_is_reproducible(tiny, prompt):
    kw = dict(max_new_tokens=5, prompt_lens=[9, 4], pad_token_id=1, seed=8, **SAMPLE)
    tokens, lens = tiny.generate(prompt, **kw)
    tokens2, lens2 = tiny.generate(prompt, **kw)
    assert torch.equal(tokens, tokens2) and torch.equal(lens, lens2)
    assert lens.tolist() == [14, 9]
    assert torch.equal(tokens[1, :4], prompt[1, :4]) and (tokens[1, 9:] == 1).all()
    other, _ = tiny.generate(prompt, **dict(kw, seed=9))
    assert not torch.equal(tokens, other)


def test_generate_sampler_argument_errors(tiny, prompt):
    with pytest.raises(ValueError):  # nucleus sampling needs the philox sampler
        tiny.generate(prompt, max_new_tokens=2, temperature=0.8, top_p=0.9, seed=1)
    with pytest.raises(ValueError):  # no seed
        tiny.generate(prompt, max_new_tokens=2, temperature=0.8, sampler="philox")
    with pytest.raises(ValueError):  # greedy is not a philox mode
        tiny.generate(prompt, max_new_tokens=2, seed=1, sampler="philox")
    with pytest.raises(ValueError):
        tiny.generate(prompt, max_new_tokens=2, sampler="dice")


# ---------------------------------------------------------------------------
# executor
# ---------------------------------------------------------------------------

class UDSHttpServer(socketserver.ThreadingUnixStreamServer):
    daemon_threads = True


def test_infer_executor_philox_end_to_end(short_tmp_path):
    from safetensors.torch import load_file, save_file

    tmp_path = short_tmp_path  # bridge.sock: a Unix socket path holds < 108 bytes
    seq_len, new = 12, 5
    ids = torch.randint(4, 512, (2, seq_len), generator=torch.Generator().manual_seed(1))
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
        "model": "llama-tiny", "data": {"any": "ref"},
        "batch_size": 2, "seq_len": seq_len, "max_new_tokens": new, "num_batches": 1,
        "sampler": "philox", "temperature": 0.8, "top_k": 20, "top_p": 0.9, "seed": 3,
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
    assert torch.equal(out["tokens"][:, :seq_len], ids)
    if not torch.cuda.is_available():
        # the executor seeds the same fp32 model on the CPU
        torch.manual_seed(3)
        model = models.build("llama-tiny").eval()
        want = model.generate(ids, max_new_tokens=new, temperature=0.8, top_k=20,
                              top_p=0.9, seed=3, sampler="philox")
        assert torch.equal(out["tokens"], want)
