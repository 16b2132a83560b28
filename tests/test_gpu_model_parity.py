"""Whole-model logits, loss and gradients on the GPU against textbook fp64.

Every HIP kernel has its own edge-shape tests; these check the MODELS built
from them, where the wiring can go wrong: the (residual, delta) pair carry,
_AddRMSNorm.backward's one dx for two inputs, checkpointing around
forward_pair, tied embeddings, bshd RoPE + GQA attention, the MoE
gather/scatter, GraphedDecoder._step's hand-written block, the GPT-2 cache
branch, RaggedStep and the paged routes.

Method (tests/model_ref64.py; its CPU checks are tests/test_model_ref64.py):
weights are re-initialised to unit gain so attention reaches the logits, the
reference is a textbook fp64 forward that shares no code with the models, and
each configuration runs twice on the GPU in bf16:

  native     the code under test (ops.has_native(), HYPHA_FORCE_REF unset);
  yardstick  HYPHA_FORCE_REF=1: PyTorch's bf16 ops on the same GPU and the
             same GEMM library, i.e. what bf16 rounding alone costs here.

Bound: every native error (logits rel-L2, worst logits row, each parameter's
gradient rel-L2) <= 2 x the yardstick's error on the same inputs. The native
kernels keep fp32 between fused steps where the yardstick rounds after every
op, so native is expected BELOW the yardstick; the factor 2 covers the scatter
of a max-type statistic between two rounding orders. test_model_ref64.py shows
on the CPU that last-layer attention faults exceed this bound. The loss must
lie within one bf16 ulp (2^-8 relative) of the fp64 loss.

Every test prints its figures as `PARITY | ...` lines (pytest -s);
profiles/model_parity.md holds those of one MI355X run.
"""

import pytest
import torch

import model_ref64 as R
from hypha_amd import models, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
FACTOR = 2.0
LOSS_TOL = 2.0 ** -8
ROUTING_MIN = 0.95

_cache: dict = {}


def prepared(name):
    """(bf16 GPU model, fp64 parameters, ids, labels) of one configuration,
    built once per session. The fp64 parameters are the model's bf16 values."""
    if name not in _cache:
        reg, kw, s = R.CONFIGS[name]
        cpu = R.unit_gain_(models.build(reg, **kw), R.SEEDS[name])
        P = R.params64(cpu)
        ids, labels = R.make_batch(cpu.cfg.vocab_size, R.BATCH, s, R.SEEDS[name] + 1)
        model = cpu.to(DEV).bfloat16()
        for buf in model.buffers():  # rope tables stay fp32
            if buf.dtype is torch.bfloat16:
                buf.data = buf.data.float()
        for n, p in model.named_parameters():  # both sides hold the same numbers
            assert torch.equal(p.detach().cpu().double(), P[n]), n
        _cache[name] = (model, P, ids, labels)
    return _cache[name]


def native(monkeypatch):
    monkeypatch.delenv("HYPHA_FORCE_REF", raising=False)
    assert ops.has_native() and ops.use_native(torch.empty(1, device=DEV))


def yardstick(monkeypatch):
    monkeypatch.setenv("HYPHA_FORCE_REF", "1")
    assert not ops.use_native(torch.empty(1, device=DEV))


def report(part, config, metric, nat, yard):
    print(f"PARITY | {part} | {config} | {metric} | native {nat:.3e} | "
          f"yardstick {yard:.3e} | ratio {nat / yard if yard else float('inf'):.2f}")


# ---- part 3: training parity ------------------------------------------------


def leaves(P):
    """A copy of P whose parameters are fresh autograd leaves."""
    return {n: (t.clone().requires_grad_(True) if not n.startswith("rope_") else t)
            for n, t in P.items()}


def textbook_train(name):
    """(logits64, loss64, grads64) of a dense configuration, computed once."""
    key = (name, "train64")
    if key not in _cache:
        model, P, ids, labels = prepared(name)
        Q = leaves(P)
        logits, loss = R.TEXTBOOK[name](Q, model.cfg, ids, labels)
        loss.backward()
        _cache[key] = (logits.detach(), loss.item(),
                       {n: Q[n].grad for n, _ in model.named_parameters()})
    return _cache[key]


def textbook_moe(routing, training, grads):
    """moe64 on M1 under a captured routing; cached per routing, so the native
    and the yardstick run share one fp64 pass whenever they route alike."""
    model, P, ids, labels = prepared("M1")
    key = ("M1", training, grads) + tuple(r.numpy().tobytes() for r in routing)
    if key not in _cache:
        Q = leaves(P) if grads else P
        with torch.set_grad_enabled(grads):
            logits, loss, own = R.moe64(Q, model.cfg, ids, labels, routing=routing,
                                        training=training)
        g = None
        if grads:
            loss.backward()
            g = {n: Q[n].grad for n, _ in model.named_parameters()}
        _cache[key] = (logits.detach(), loss.item(), g, own)
    return _cache[key]


class Routing:
    """Forward hooks on every mlp.router: the routing of the LAST forward, by
    the model's own rule (fp32 softmax of the router's output, then top-k)."""

    def __init__(self, model):
        self.model, self.sets = model, {}
        self.handles = [blk.mlp.router.register_forward_hook(self._hook(i))
                        for i, blk in enumerate(model.blocks)]

    def _hook(self, i):
        def f(mod, inp, out):
            self.sets[i] = R.topk_sets(out, self.model.cfg.top_k)
        return f

    def take(self):
        return [self.sets[i] for i in range(len(self.handles))]

    def close(self):
        for h in self.handles:
            h.remove()


def train_run(model, ids, labels, routing=None):
    """One bf16 training step's outputs: (logits, loss, grads[, routings])."""
    model.train()
    model.zero_grad(set_to_none=True)
    ids, labels = ids.to(DEV), labels.to(DEV)
    with torch.no_grad():
        logits = model(ids).float().cpu()
    r_logits = routing.take() if routing else None
    loss = model(ids, labels=labels)
    loss.backward()
    r_loss = routing.take() if routing else None
    torch.cuda.synchronize()
    grads = {n: p.grad.float().cpu() for n, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    return logits, loss.item(), grads, r_logits, r_loss


def compare_training(config, nat, yard, ref_nat, ref_yard):
    """nat/yard: (logits, loss, grads) of the two runs; ref_*: the textbook's
    (logits64, loss64, grads64) each is judged against."""
    failures = []

    def bound(metric, a, b):
        report("training", config, metric, a, b)
        if not a <= FACTOR * b:
            failures.append(f"{metric}: native {a:.3e} > {FACTOR} x yardstick {b:.3e}")

    bound("logits rel_l2", R.rel_l2(nat[0], ref_nat[0]), R.rel_l2(yard[0], ref_yard[0]))
    bound("logits worst_row", R.worst_row(nat[0], ref_nat[0]),
          R.worst_row(yard[0], ref_yard[0]))
    e_nat = R.grad_rel_l2(nat[2], ref_nat[2])
    e_yard = R.grad_rel_l2(yard[2], ref_yard[2])
    for n in e_nat:
        g = nat[2][n]
        if not torch.isfinite(g).all():
            failures.append(f"grad {n}: not finite")
        if ref_nat[2][n].abs().max() > 0 and g.abs().max() == 0:
            failures.append(f"grad {n}: all zero, the textbook's is not")
        bound(f"grad {n}", e_nat[n], e_yard[n])
    worst = max(e_nat, key=lambda n: e_nat[n] / e_yard[n] if e_yard[n] else float("inf"))
    report("training", config, f"worst grad ratio ({worst})", e_nat[worst], e_yard[worst])
    for who, run, ref in (("native", nat, ref_nat), ("yardstick", yard, ref_yard)):
        err = abs(run[1] - ref[1]) / abs(ref[1])
        print(f"PARITY | training | {config} | loss | {who} {run[1]:.6f} | "
              f"fp64 {ref[1]:.6f} | rel {err:.3e} | bound {LOSS_TOL:.3e}")
        if who == "native" and not err <= LOSS_TOL:
            failures.append(f"loss: {run[1]} vs fp64 {ref[1]}, rel {err:.3e}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", ["L1", "L2", "G1"])
def test_training_parity(monkeypatch, name):
    model, P, ids, labels = prepared(name)
    ref = textbook_train(name)
    native(monkeypatch)
    nat = train_run(model, ids, labels)
    yardstick(monkeypatch)
    yard = train_run(model, ids, labels)
    compare_training(name, nat, yard, ref, ref)


def check_routing(config, who, captured, own):
    """The condition of every MoE comparison: the run routed as fp64 would for
    at least ROUTING_MIN of the tokens in every layer."""
    for i, (c, o) in enumerate(zip(captured, own)):
        agree = R.routing_agreement(c, o)
        print(f"PARITY | routing | {config} | layer {i} | {who} {agree:.4f} | "
              f"min {ROUTING_MIN}")
        assert agree >= ROUTING_MIN, (config, who, i, agree)


def test_training_parity_moe(monkeypatch):
    """M1 in training mode: CE + Switch aux loss, and every gradient. Each run
    is judged against the textbook under that run's own routing."""
    model, P, ids, labels = prepared("M1")
    routing = Routing(model)
    try:
        native(monkeypatch)
        nat = train_run(model, ids, labels, routing)
        yardstick(monkeypatch)
        yard = train_run(model, ids, labels, routing)
    finally:
        routing.close()
    refs = []
    for who, run in (("native", nat), ("yardstick", yard)):
        lg, _, _, own = textbook_moe(run[3], True, False)  # the logits forward
        check_routing("M1 train", who, run[3], own)
        _, loss, grads, own = textbook_moe(run[4], True, True)  # the loss forward
        check_routing("M1 train", who, run[4], own)
        refs.append((lg, loss, grads))
    compare_training("M1 train", nat, yard, *refs)


@pytest.mark.parametrize("grouped", [False, True], ids=["library", "native_grouped"])
def test_eval_parity_moe(monkeypatch, grouped):
    """M1 in eval mode, logits only; once through the per-expert library loop
    and once through the native grouped-GEMM kernel (HYPHA_NATIVE_GROUPED=1)."""
    from hypha_amd import _C

    model, P, ids, labels = prepared("M1")
    config = "M1 eval grouped" if grouped else "M1 eval"
    calls = []
    real = _C.grouped_gemm
    monkeypatch.setattr(_C, "grouped_gemm", lambda *a: (calls.append(1), real(*a))[1])
    routing = Routing(model)
    runs = {}
    try:
        model.eval()
        for who in ("native", "yardstick"):
            if who == "native":
                native(monkeypatch)
                monkeypatch.setenv("HYPHA_NATIVE_GROUPED", "1" if grouped else "0")
            else:
                yardstick(monkeypatch)  # the grouped kernel is no yardstick
                monkeypatch.setenv("HYPHA_NATIVE_GROUPED", "0")
            n0 = len(calls)
            with torch.no_grad():
                logits = model(ids.to(DEV)).float().cpu()
            want = 3 * model.cfg.n_layers if grouped and who == "native" else 0
            assert len(calls) - n0 == want, (who, len(calls) - n0)
            runs[who] = (logits, routing.take())
    finally:
        routing.close()
    err = {}
    for who, (logits, sets) in runs.items():
        lg64, _, _, own = textbook_moe(sets, False, False)
        check_routing(config, who, sets, own)
        err[who] = (R.rel_l2(logits, lg64), R.worst_row(logits, lg64))
    for k, metric in enumerate(("logits rel_l2", "logits worst_row")):
        report("training", config, metric, err["native"][k], err["yardstick"][k])
    assert err["native"][0] <= FACTOR * err["yardstick"][0]
    assert err["native"][1] <= FACTOR * err["yardstick"][1]


# ---- part 4: generation routes, judged by the logits that chose each token --


def prompts(vocab, lens, s, seed):
    """ids [B, s]: sequence b holds lens[b] random tokens, then the pad token."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, vocab, (len(lens), s), generator=g)
    for b, n in enumerate(lens):
        ids[b, n:] = 0
    return ids.to(DEV)


def lm_head_recorder(model, rec):
    return model.lm_head.register_forward_hook(
        lambda mod, inp, out: rec.append(out[:, 0].float().cpu()))


def route_generate(model, lens, s, new, **kw):
    """model.generate; returns (tokens [B, s + new], one [B, V] per step)."""
    rec = []
    ids = prompts(model.cfg.vocab_size, lens, s, seed=11)
    handle = lm_head_recorder(model, rec)
    try:
        if len(set(lens)) > 1 or "kv_layout" in kw:
            tokens, out_lens = model.generate(ids, max_new_tokens=new, prompt_lens=lens,
                                              pad_token_id=0, **kw)
            assert out_lens.tolist() == [n + new for n in lens]
        else:
            tokens = model.generate(ids, max_new_tokens=new, **kw)
    finally:
        handle.remove()
    return tokens, rec


def route_graphed(model, lens, s, new, ragged, **kw):
    """GraphedDecoder.generate below the capture threshold (eager _step /
    _step_ragged); the logits are those handed to dec._pick."""
    from hypha_amd.runtime.graphed_decode import GraphedDecoder

    rec = []
    ids = prompts(model.cfg.vocab_size, lens, s, seed=11)
    dec = GraphedDecoder(model, batch=len(lens), prompt_len=s, max_new=new, **kw)
    pick = dec._pick

    def recording_pick(logits, sample):
        rec.append(logits.float().cpu())
        return pick(logits, sample)

    dec._pick = recording_pick
    if ragged:
        tokens, out_lens = dec.generate(ids, max_new_tokens=new, prompt_lens=lens,
                                        pad_token_id=0)
        assert out_lens.tolist() == [n + new for n in lens]
    else:
        tokens = dec.generate(ids, max_new_tokens=new)
    # below 8 new tokens nothing is captured: every step ran eagerly
    assert new < 8 and all(g is None for g in (dec.graph, dec.graph_r, dec.graph_s,
                                               dec.graph_rs))
    return tokens, rec


RAGGED = [61, 3, 64]
REVERSED5 = [4, 3, 2, 1, 0]  # pages of [61, 3, 64] + 6 rows: 2 + 1 + 2

# route -> (lens, s, new, runner)
ROUTES = {
    "generate_s128": ([128, 128], 128, 4, lambda m, *a: route_generate(m, *a)),
    "generate_s61": ([61, 61], 61, 6, lambda m, *a: route_generate(m, *a)),
    "generate_s61_chunk24": ([61, 61], 61, 6,
                             lambda m, *a: route_generate(m, *a, prefill_chunk=24)),
    "ragged": (RAGGED, 64, 6, lambda m, *a: route_generate(m, *a)),
    "ragged_paged": (RAGGED, 64, 6,
                     lambda m, *a: route_generate(m, *a, kv_layout="paged",
                                                  kv_free_order=REVERSED5)),
    "graphed_uniform": ([61, 61], 61, 7, lambda m, *a: route_graphed(m, *a, False)),
    "graphed_ragged": ([61, 3, 33], 61, 7, lambda m, *a: route_graphed(m, *a, True)),
    # 3 sequences x ceil(68 / 64) = 2 pages each, handed out last page first
    "graphed_paged": ([61, 3, 33], 61, 7,
                      lambda m, *a: route_graphed(m, *a, True, kv_layout="paged",
                                                  kv_free_order=[5, 4, 3, 2, 1, 0])),
}


def compare_route(monkeypatch, config, route, model, P, tokens, rec, lens, new):
    """Step i of sequence b against the textbook's row L_b + i - 1 over the
    tokens that were produced (so a greedy flip cannot matter); the yardstick
    is the HYPHA_FORCE_REF=1 full forward over the same tokens, same rows."""
    assert len(rec) == new, (len(rec), new)
    textbook = R.TEXTBOOK[config]
    got, yard, want = [], [], []
    yardstick(monkeypatch)
    model.eval()
    for b, n in enumerate(lens):
        seq = tokens[b, :n + new]
        rows = torch.arange(n - 1, n + new - 1)
        with torch.no_grad():
            want.append(textbook(P, model.cfg, seq.cpu()[None])[0][0, rows])
            yard.append(model(seq[None])[0].float().cpu()[rows])
        got.append(torch.stack([rec[i][b] for i in range(new)]))
    got, yard, want = torch.cat(got), torch.cat(yard), torch.cat(want)
    e_nat, e_yard = R.worst_row(got, want), R.worst_row(yard, want)
    report("generation", config, f"{route} worst_row over {got.shape[0]} rows",
           e_nat, e_yard)
    assert torch.isfinite(got).all()
    assert e_nat <= FACTOR * e_yard, (config, route, e_nat, e_yard)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("config", ["L1", "L2u"])
def test_generation_route_logits(monkeypatch, config, route):
    model, P, _, _ = prepared(config)
    lens, s, new, run = ROUTES[route]
    native(monkeypatch)
    tokens, rec = run(model.eval(), lens, s, new)
    compare_route(monkeypatch, config, route, model, P, tokens, rec, lens, new)


@pytest.mark.parametrize("kw", [{}, {"prefill_chunk": 24}], ids=["s61", "s61_chunk24"])
def test_generation_route_logits_gpt2(monkeypatch, kw):
    """G1's cache branch: attn_prefill with a ragged tail (and pos > 0 when
    chunked), then decode across row 64. The logits are rebuilt from ln_f's
    output as generate() builds them (tied head)."""
    model, P, _, _ = prepared("G1")
    lens, s, new = [61, 61], 61, 6
    rec = []
    ids = prompts(model.cfg.vocab_size, lens, s, seed=11)
    native(monkeypatch)
    handle = model.ln_f.register_forward_hook(
        lambda mod, inp, out: rec.append(
            torch.nn.functional.linear(out, model.wte.weight)[:, 0].float().cpu()))
    try:
        tokens = model.eval().generate(ids, max_new_tokens=new, **kw)
    finally:
        handle.remove()
    compare_route(monkeypatch, "G1", "generate_" + "_".join(["s61"] + [
        f"chunk{v}" for v in kw.values()]), model, P, tokens, rec, lens, new)
