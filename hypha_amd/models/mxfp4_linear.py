"""Weight-only MXFP4 linears for serving: each weight is an e2m1 code, two per
byte, with one E8M0 power-of-two scale per 32 consecutive inputs of a row
(ops.quantize_mxfp4, the OCP microscaling format), 4.25 bits per weight
against bf16's 16, and applied by ops.linear_mxfp4w: the weight-streaming HIP
kernel for decode-sized batches, dequantise + library for prefill. The experts
of the MoE family are quantised the same way by MoEMLP.quantize_experts_mxfp4_
and applied by ops.moe_ffn_mxfp4w. Both take an optional act_quant="mxfp8",
which rounds their activations to MXFP8 and runs the block-scaled MFMA
kernels. Inference only."""

from __future__ import annotations

import torch
import torch.nn as nn

from hypha_amd import ops


class Mxfp4Linear(nn.Module):
    """Bias-free linear on codes (uint8 [out, in / 2]) and scales (uint8
    [out, in / 32]); W = ops.dequantize_mxfp4(codes, scales). Both buffers are
    integers, so .to(dtype) and .bfloat16() only ever move them. act_quant is
    ops.linear_mxfp4w's: None, or "mxfp8" to round the activations to MXFP8
    and take the block-scaled MFMA kernel."""

    def __init__(self, codes: torch.Tensor, scales: torch.Tensor, act_quant: str | None = None):
        super().__init__()
        self.act_quant = act_quant
        self.out_features, self.in_features = codes.shape[0], 2 * codes.shape[1]
        self.register_buffer("codes", codes)
        self.register_buffer("scales", scales)

    @classmethod
    @torch.no_grad()
    def from_linear(cls, lin: nn.Linear, act_quant: str | None = None) -> "Mxfp4Linear":
        if lin.bias is not None:
            raise ValueError("Mxfp4Linear has no bias")
        return cls(*ops.quantize_mxfp4(lin.weight.detach()), act_quant=act_quant)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.linear_mxfp4w(x, self.codes, self.scales, act_quant=self.act_quant)

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, "
                f"act_quant={self.act_quant!r}")


@torch.no_grad()
def quantize_linears_mxfp4_(model: nn.Module, act_quant: str | None = None,
                            expert_act_quant: str | None = None) -> nn.Module:
    """Replace, in place, every bias-free nn.Linear whose shape
    ops/hip/linear_mxfp4w.hip serves by an Mxfp4Linear (in the Llama family:
    wq, wk, wv, wo, w_gate, w_up, w_down and an untied lm_head). A linear that
    shares its weight with an embedding (a tied head), one with a bias and one
    of another shape stay as they are: the rules of quantize_linears_fp8_. The
    experts of every MoEMLP whose shapes ops.moe_ffn_mxfp4w serves are
    quantised the same way (MoEMLP.quantize_experts_mxfp4_); its router is a
    linear like any other (with 8 outputs it is of another shape and stays
    bf16). act_quant is set on the linears created and on the Mxfp4Linears
    already there and leaves the experts weight-only; expert_act_quant is
    the experts' own mode (MoEMLP.act_quant: "mxfp8" rounds the activations of
    both stages of the expert FFN to MXFP8), set on every such MoEMLP, the
    ones already quantised included. Returns the model in eval mode."""
    from .moe import MoEMLP

    if act_quant not in (None, "mxfp8"):
        raise ValueError(f"act_quant must be None or 'mxfp8', got {act_quant!r}")
    if expert_act_quant not in (None, "mxfp8"):
        raise ValueError(f"expert_act_quant must be None or 'mxfp8', got {expert_act_quant!r}")

    tied = {id(m.weight) for m in model.modules() if isinstance(m, nn.Embedding)}
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if (isinstance(child, nn.Linear) and child.bias is None
                    and id(child.weight) not in tied
                    and ops.linear_mxfp4w_native_shapes(*child.weight.shape)):
                setattr(parent, name, Mxfp4Linear.from_linear(child, act_quant))
            elif isinstance(child, Mxfp4Linear):
                child.act_quant = act_quant
        if isinstance(parent, MoEMLP) and ops.moe_ffn_native_shapes(
                parent.cfg.hidden_size, parent.cfg.ffn_hidden, parent.cfg.n_experts,
                parent.cfg.top_k):
            parent.quantize_experts_mxfp4_(expert_act_quant)
    return model.eval()
