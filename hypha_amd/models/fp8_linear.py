"""Weight-only fp8 linears for serving: each weight row is stored as e4m3
codes with one fp32 scale (ops.quantize_rows_e4m3), half the bytes of bf16,
and applied by ops.linear_fp8w: the weight-streaming HIP kernel for
decode-sized batches, dequantise + library for prefill. The experts of the MoE
family are quantised the same way by MoEMLP.quantize_experts_fp8_ and applied
by ops.moe_ffn_fp8w. Inference only."""

from __future__ import annotations

import torch
import torch.nn as nn

from hypha_amd import ops


class Fp8Linear(nn.Module):
    """Bias-free linear on weight8 (float8_e4m3fn [out, in]) and scale (fp32
    [out]); W = weight8 * scale[:, None]."""

    def __init__(self, weight8: torch.Tensor, scale: torch.Tensor):
        super().__init__()
        self.out_features, self.in_features = weight8.shape
        self.register_buffer("weight8", weight8)
        self.register_buffer("scale", scale)

    @classmethod
    @torch.no_grad()
    def from_linear(cls, lin: nn.Linear) -> "Fp8Linear":
        if lin.bias is not None:
            raise ValueError("Fp8Linear has no bias")
        return cls(*ops.quantize_rows_e4m3(lin.weight.detach()))

    def _apply(self, fn, recurse=True):
        # .to(dtype) / .bfloat16() cast every floating buffer; the codes and
        # their fp32 scales must only ever move, so they pass as integers
        self._buffers["weight8"] = fn(self.weight8.view(torch.uint8)).view(torch.float8_e4m3fn)
        self._buffers["scale"] = fn(self.scale.view(torch.int32)).view(torch.float32)
        return self

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.linear_fp8w(x, self.weight8, self.scale)

    def extra_repr(self) -> str:
        return f"in_features={self.in_features}, out_features={self.out_features}"


@torch.no_grad()
def quantize_linears_fp8_(model: nn.Module) -> nn.Module:
    """Replace, in place, every bias-free nn.Linear whose shape
    ops/hip/linear_fp8w.hip serves by an Fp8Linear (in the Llama family: wq,
    wk, wv, wo, w_gate, w_up, w_down and an untied lm_head). A linear that
    shares its weight with an embedding (a tied head), one with a bias and one
    of another shape stay as they are. The experts of every MoEMLP whose
    shapes ops.moe_ffn_fp8w serves are quantised the same way
    (MoEMLP.quantize_experts_fp8_); its router is a linear like any other
    (with 8 outputs it is of another shape and stays bf16). Returns the model
    in eval mode."""
    from .moe import MoEMLP

    tied = {id(m.weight) for m in model.modules() if isinstance(m, nn.Embedding)}
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if (isinstance(child, nn.Linear) and child.bias is None
                    and id(child.weight) not in tied
                    and ops.linear_fp8w_native_shapes(*child.weight.shape)):
                setattr(parent, name, Fp8Linear.from_linear(child))
        if isinstance(parent, MoEMLP) and ops.moe_ffn_native_shapes(
                parent.cfg.hidden_size, parent.cfg.ffn_hidden, parent.cfg.n_experts,
                parent.cfg.top_k):
            parent.quantize_experts_fp8_()
    return model.eval()


def check_weight_quant(weight_quant) -> None:
    if weight_quant not in (None, "fp8", "mxfp4", "mxfp4_a8", "mxfp4_experts_a8"):
        raise ValueError("weight_quant must be None, 'fp8', 'mxfp4', 'mxfp4_a8' or "
                         f"'mxfp4_experts_a8', got {weight_quant!r}")
