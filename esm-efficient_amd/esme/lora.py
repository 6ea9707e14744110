"""LoRA adapters for inference on the packed forward (reference `esme/lora.py`: same names, arguments, attributes and
state-dict keys, so adapter files written by the reference's `save_lora` load unchanged).

    y = W x + b + sum_n (alpha / rank) B_n (A_n x)        A_n (rank, in), B_n (out, rank), n over the selected adapter names

Nothing here merges B A into the bf16 weight (re-rounding W + s B A to 8 significant bits would discard most of a small delta, and
the adapters could no longer be selected per call).  The delta rides in an EXTENSION K-TILE of the projection's own GEMM instead:

    [x | u] [W | s B]^T = x W^T + u (s B)^T,        u = x A^T   (esme_hip_lora_down, written next to x in the same buffer)

so it accumulates in fp32 inside the MFMA chain and every fused epilogue of the hot path (LayerNorm fold, rotary, q pre-scale,
residual, row statistics, GELU, SwiGLU) is untouched (esme/lora_fused.py, esme/attention.py).  The wrapped projections are the
reference's four (q, k, v, out of the attention block) and, beyond it, the FFN's (`ESM2.add_lora(layers=(..., 'ffn_up', 'ffn_down'))`:
the up-projection -- SwiGLU: its gate and fc, one wrapper each -- and the down-projection, whose adapter reads K = the FFN width).
That fused forward is for inference: it has no
backward, dropout is stored and ignored in eval(), a forward in train() raises.  Adapters are trained through
`model.forward_trainable` (esme/autograd.py), the reference's unfused data flow with a grad_fn.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import torch
from torch import nn

from esme import _hip
from esme.nn import Derived, version_key

EXT_TILE = 64            # the GEMM's K tile: extension widths are multiples of it
MAX_EXT = 256            # widest extension esme_hip_lora_down is built for
INFERENCE_ONLY = 'LoRA adapters run for inference only: call model.eval() (no backward, no dropout)'     # (raised here and by esme.lora_fused.check_mode)


def ext_width(rows: int) -> int:
    """Extension columns that hold `rows` stacked adapter rows (NotImplementedError past what the kernel is built for)."""
    X = (rows + EXT_TILE - 1) // EXT_TILE * EXT_TILE
    if X > MAX_EXT:
        raise NotImplementedError(f'LoRA: {rows} active adapter rows in one projection GEMM need an extension of {X} columns; '
                                  f'this build serves up to {MAX_EXT} (select fewer adapters with lora_names=, or lower ranks)')
    return X


class LoRA(nn.Module):
    """A projection with named low-rank adapters: `layer` (the wrapped Linear), `lora_A[name]` (rank, in), `lora_B[name]` (out, rank)."""

    def __init__(self, layer: nn.Module, rank: int = 16, alpha: int = 1, dropout_p: float = 0., names: Optional[list] = None, dtype=None):
        super().__init__()
        assert getattr(layer, 'in_features', None) is not None, 'The layer must have an attribute in_features'
        assert getattr(layer, 'out_features', None) is not None, 'The layer must have an attribute out_features'
        assert rank >= 0, 'The rank must be a non-negative integer'
        if rank == 0:
            raise NotImplementedError('LoRA: rank 0 has no adapter to run (ranks 1 .. 64 are served)')
        self.layer = layer
        self.rank, self.alpha, self.dropout_p = rank, alpha, dropout_p
        self.scaling = self.alpha / self.rank
        self.in_features, self.out_features = layer.in_features, layer.out_features
        names = list(names or ['default'])
        self.names = set(names)
        ref = layer.weight
        dtype = dtype or ref.dtype
        if dtype in (torch.uint8, torch.int8):
            dtype = torch.bfloat16
        self.lora_A = nn.ParameterDict({n: nn.Parameter(torch.zeros(rank, self.in_features, device=ref.device, dtype=dtype)) for n in names})
        self.lora_B = nn.ParameterDict({n: nn.Parameter(torch.zeros(self.out_features, rank, device=ref.device, dtype=dtype)) for n in names})
        self.reset_parameters()
        self._derived = Derived()         # 'ext': ([W | s B | 0], stacked A), the standalone forward's weights

    def reset_parameters(self):
        for n in self.lora_A:
            if self.lora_A[n].is_meta:
                continue
            nn.init.kaiming_uniform_(self.lora_A[n], a=math.sqrt(5))
            nn.init.zeros_(self.lora_B[n])

    # the wrapped projection's parameters under the names the weight-packing code reads them by
    @property
    def weight(self):
        return self.layer.weight

    @property
    def bias(self):
        return self.layer.bias

    def select(self, names=None) -> tuple:
        """The adapters a call applies, in order: every adapter (insertion order) for None / an empty list, else the names given.
        KeyError for a name this projection does not have."""
        if not names:
            return tuple(self.lora_A.keys())
        names = tuple(names)
        for n in names:
            if n not in self.lora_A:
                raise KeyError(f'LoRA adapter {n!r} not found (available: {sorted(self.lora_A.keys())})')
        return names

    def stacked(self, names: tuple):
        """(A (len(names) * rank, in) bf16, [s B_n ...] (out, len(names) * rank) fp32) of the selected adapters."""
        A = torch.cat([self.lora_A[n].data.to(torch.bfloat16) for n in names], dim=0)
        B = torch.cat([self.lora_B[n].data.float() * float(self.scaling) for n in names], dim=1)
        return A, B

    def params(self, names: tuple):
        return [p for n in names for p in (self.lora_A[n], self.lora_B[n])]

    def stage_form(self, names=None):
        """([W | s B | 0] (out, in + X) bf16, stacked A) of the adapters `names` (select()): the operands of the standalone forward."""
        names = self.select(names)
        w = self.layer.weight
        if w.dtype != torch.bfloat16:
            raise NotImplementedError('LoRA adapters need unquantised bfloat16 base weights (quantization= is not supported with adapters)')
        return self._derived.get('ext', (names, float(self.scaling), version_key(w, *self.params(names))), self._build_stage_form, names)

    def _build_stage_form(self, names: tuple):
        w = self.layer.weight
        A, B = self.stacked(names)
        K, X = w.shape[1], ext_width(A.shape[0])
        we = torch.zeros(w.shape[0], K + X, dtype=torch.bfloat16, device=w.device)
        we[:, :K] = w.data
        we[:, K:K + B.shape[1]] = B.to(torch.bfloat16)
        return we, A.contiguous()

    def forward(self, x: torch.Tensor, names=None):
        """layer(x) + sum_n scaling * B_n A_n x as ONE GEMM over [x | x A^T] (the stage form; the model's hot path fuses the
        adapters of q, k and v into its packed QKV GEMM: esme.attention.FlashMultiheadAttention)."""
        if self.training:
            raise NotImplementedError(INFERENCE_ONLY)
        (we, A), b = self.stage_form(names), self.layer.bias
        shape = x.shape
        x2 = x.reshape(-1, shape[-1])
        K, X = x2.shape[1], we.shape[1] - x2.shape[1]
        xe = torch.empty(x2.shape[0], K + X, dtype=torch.bfloat16, device=x.device)
        xe[:, :K].copy_(x2)                                   # (row move, no arithmetic)
        _hip.lora_down(xe[:, :K], A, xe[:, K:])
        y = _hip.gemm(xe, we, b)
        return y if x.dim() == 2 else y.view(*shape[:-1], y.shape[-1])

    def extra_repr(self):
        return f'in_features={self.in_features}, out_features={self.out_features}, rank={self.rank}, alpha={self.alpha}, dropout_p={self.dropout_p}'


def _is_lora_key(k: str) -> bool:
    return '.lora_A.' in k or '.lora_B.' in k


def mark_only_lora_as_trainable(model: nn.Module, names=None) -> None:
    """requires_grad = True on the adapters (all, or those called `names`), False on every other parameter."""
    names = set(names or [])
    for k, p in model.named_parameters():
        p.requires_grad = _is_lora_key(k) and (not names or k.rsplit('.', 1)[-1] in names)


def lora_state_dict(model: nn.Module, names=None) -> Dict[str, torch.Tensor]:
    """The adapter tensors of model.state_dict() (all, or those called `names`)."""
    names = set(names or [])
    return {k: v for k, v in model.state_dict().items() if _is_lora_key(k) and (not names or k.rsplit('.', 1)[-1] in names)}


def lora_modules(model: nn.Module):
    return [m for m in model.modules() if isinstance(m, LoRA)]
