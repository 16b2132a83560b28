"""The textbook fp64 references of tests/model_ref64.py, checked on the CPU.

1. Each model's own fp32 CPU path agrees with its textbook to rel-L2 <= 1e-5
   on logits, loss and every gradient, at the configurations the GPU parity
   tests use: the references are right, and so is the Python wiring (pair
   carry, checkpointing, tied head, MoE gather/scatter) on the CPU.
2. The metric and the bound of the GPU tests can see a wrong kernel: four
   faults, each in the last layer's attention only, move the worst logits row
   by more than twice what the bf16 path's rounding does.
"""

import math

import pytest
import torch

import model_ref64 as R
from hypha_amd import models

TOL = 1e-5


def build_unit(name):
    reg, kw, s = R.CONFIGS[name]
    model = R.unit_gain_(models.build(reg, **kw), R.SEEDS[name]).train()
    ids, labels = R.make_batch(model.cfg.vocab_size, R.BATCH, s, R.SEEDS[name] + 1)
    return model, ids, labels


def capture_routing(model, store):
    """Forward hooks that record every layer's routing of the LAST forward."""
    def hook(i):
        def f(mod, inp, out):
            store[i] = R.topk_sets(out, model.cfg.top_k)
        return f
    return [blk.mlp.router.register_forward_hook(hook(i))
            for i, blk in enumerate(model.blocks)]


@pytest.mark.parametrize("name", ["L1", "L2", "G1", "M1"])
def test_cpu_fp32_path_matches_textbook(name):
    model, ids, labels = build_unit(name)
    routing = {}
    if name == "M1":
        capture_routing(model, routing)
    logits = model(ids).detach()
    loss = model(ids, labels=labels)
    loss.backward()

    P = R.params64(model, requires_grad=True)
    if name == "M1":
        lg64, loss64, own = R.moe64(P, model.cfg, ids, labels,
                                    routing=[routing[i] for i in range(model.cfg.n_layers)],
                                    training=True)
        for i, o in enumerate(own):
            agree = R.routing_agreement(routing[i], o)
            print(f"{name} layer {i}: fp32 routing == fp64 routing for {agree:.4f} of tokens")
    else:
        lg64, loss64 = R.TEXTBOOK[name](P, model.cfg, ids, labels)
    loss64.backward()

    e_logits = R.rel_l2(logits, lg64)
    e_loss = abs(loss.item() - loss64.item()) / abs(loss64.item())
    grads = R.grad_rel_l2({n: p.grad for n, p in model.named_parameters()},
                          {n: P[n].grad for n, _ in model.named_parameters()})
    worst = max(grads, key=grads.get)
    print(f"{name}: logits {e_logits:.2e} loss {e_loss:.2e} "
          f"worst grad {grads[worst]:.2e} ({worst})")
    assert e_logits <= TOL
    assert e_loss <= TOL
    for n, e in grads.items():
        assert e <= TOL, (n, e)


def test_moe_seed_routes_like_fp64_in_bf16():
    """The condition of the GPU MoE comparisons holds for M1's seed on the CPU
    bf16 path: in every layer at least 95 % of the tokens choose the top-k set
    the textbook chooses in fp64 (the rest sit at near ties)."""
    model, ids, _ = build_unit("M1")
    P = R.params64(model)
    tables = model.rope_cos.clone(), model.rope_sin.clone()
    model = model.bfloat16().eval()
    model.rope_cos, model.rope_sin = tables
    routing = {}
    capture_routing(model, routing)
    with torch.no_grad():
        model(ids)
        sets = [routing[i] for i in range(model.cfg.n_layers)]
        _, _, own = R.moe64(P, model.cfg, ids, routing=sets)
    for i, o in enumerate(own):
        agree = R.routing_agreement(sets[i], o)
        print(f"M1 layer {i}: bf16 routing == fp64 routing for {agree:.4f} of tokens")
        assert agree >= 0.95


# ---- discrimination --------------------------------------------------------

FAULTS = ("k_rotated_one_late", "gqa_modulo_map", "key63_hidden_from_rows_ge_64",
          "row127_blind_to_keys_120_126")


def faulty_llama64(P, cfg, ids, fault):
    """A copy of model_ref64.llama64 with one fault in the LAST layer's attention."""
    x = P["embed.weight"][ids]
    b, s = ids.shape
    hd = cfg.hidden_size // cfg.n_heads
    rep = cfg.n_heads // cfg.n_kv_heads
    cos, sin = P["rope_cos"], P["rope_sin"]
    for i in range(cfg.n_layers):
        bad = fault if i == cfg.n_layers - 1 else None
        pre = f"blocks.{i}."
        h = R.rms64(x, P[pre + "attn_norm.weight"], cfg.norm_eps)
        q = (h @ P[pre + "attn.wq.weight"].T).view(b, s, cfg.n_heads, hd)
        k = (h @ P[pre + "attn.wk.weight"].T).view(b, s, cfg.n_kv_heads, hd)
        v = (h @ P[pre + "attn.wv.weight"].T).view(b, s, cfg.n_kv_heads, hd)
        q = R.rope64(q, cos, sin)
        k = (R.rope64(k, cos[1:], sin[1:]) if bad == "k_rotated_one_late"
             else R.rope64(k, cos, sin))
        kh, vh = k.transpose(1, 2), v.transpose(1, 2)
        if bad == "gqa_modulo_map":  # head h reads kv head h % Hkv
            kh, vh = kh.repeat(1, rep, 1, 1), vh.repeat(1, rep, 1, 1)
        else:
            kh, vh = kh.repeat_interleave(rep, 1), vh.repeat_interleave(rep, 1)
        sc = q.transpose(1, 2) @ kh.transpose(-1, -2) / math.sqrt(hd)
        mask = torch.ones(s, s, dtype=torch.bool).triu(1)
        if bad == "key63_hidden_from_rows_ge_64":
            mask[64:, 63] = True
        if bad == "row127_blind_to_keys_120_126":
            mask[127, 120:127] = True
        o = torch.softmax(sc.masked_fill(mask, float("-inf")), -1) @ vh
        x = x + o.transpose(1, 2).reshape(b, s, -1) @ P[pre + "attn.wo.weight"].T
        h = R.rms64(x, P[pre + "mlp_norm.weight"], cfg.norm_eps)
        g = h @ P[pre + "mlp.w_gate.weight"].T
        u = h @ P[pre + "mlp.w_up.weight"].T
        x = x + (torch.nn.functional.silu(g) * u) @ P[pre + "mlp.w_down.weight"].T
    return R.rms64(x, P["norm.weight"], cfg.norm_eps) @ P["lm_head.weight"].T


@pytest.fixture(scope="module")
def l1_noise():
    """(P, cfg, ids, true fp64 logits, worst_row of the CPU bf16 path)."""
    model, ids, _ = build_unit("L1")
    P = R.params64(model)
    with torch.no_grad():
        true, _ = R.llama64(P, model.cfg, ids)
        tables = model.rope_cos.clone(), model.rope_sin.clone()
        model = model.bfloat16()
        model.rope_cos, model.rope_sin = tables  # the tables stay fp32
        noise = R.worst_row(model(ids), true)
    return P, model.cfg, ids, true, noise


def test_faulty_copy_without_a_fault_is_the_textbook(l1_noise):
    P, cfg, ids, true, _ = l1_noise
    with torch.no_grad():
        assert torch.equal(faulty_llama64(P, cfg, ids, None), true)


@pytest.mark.parametrize("fault", FAULTS)
def test_bound_sees_last_layer_attention_faults(l1_noise, fault):
    """worst_row(faulty, true) > 2 * worst_row(bf16 path, true): a kernel with
    this fault cannot pass the GPU tests' bound of twice the bf16 yardstick."""
    P, cfg, ids, true, noise = l1_noise
    with torch.no_grad():
        moved = R.worst_row(faulty_llama64(P, cfg, ids, fault), true)
    print(f"{fault}: worst row {moved:.2e} vs bf16 noise {noise:.2e} "
          f"({moved / noise:.1f}x)")
    assert moved > 2 * noise
