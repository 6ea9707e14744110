"""Attention maps of chosen layers and heads from the packed forward (`model.attention_maps`).

    P^(l,h)_ij = softmax_j((q_i . k_j) * scale) over all S keys of the protein, bos / eos rows and columns included,

of the bf16 operands layer l's attention kernel consumes (post-rotary; ESM-C: post-q/k-LayerNorm) -- what fair-esm returns with
need_head_weights=True and Hugging Face with output_attentions=True, and what the reference package cannot return
(flash_attn_varlen_func gives no weights back).  The fused attention kernel never forms P; here every SELECTED layer hands its final
(q, k) to esme_hip_attn_maps (csrc/attn_maps.hip), which recomputes the scores on the MFMA and writes the normalised maps of the
selected heads, or their weighted sum, into one buffer.  `predict_contacts` / `contact_features` stay the route for a regression over
all L H heads: they store no S x S object at all.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from esme import _hip_attn_maps
from esme.qk_observer import QKObserver

DTYPES = (torch.float32, torch.bfloat16)


def select_indices(arg, n: int, what: str):
    """`layers=` / `heads=` of attention_maps as a list of indices in [0, n): None = all, negative indices count from the end.
    IndexError when one is out of range, ValueError on duplicates or an empty list."""
    if arg is None:
        return list(range(n))
    if isinstance(arg, torch.Tensor):
        arg = arg.tolist()
    if isinstance(arg, int):
        arg = [arg]
    out = []
    for i in arg:
        i = int(i)
        if not -n <= i < n:
            raise IndexError(f'attention_maps: {what} index {i} is out of range for {n} {what}')
        out.append(i % n)
    if not out:
        raise ValueError(f'attention_maps: {what} is empty (None selects all {n})')
    if len(set(out)) != len(out):
        raise ValueError(f'attention_maps: {what} holds duplicates: {list(arg)} -> {out}')
    return out


def check_head_weights(head_weights, n_layers: int, n_heads: int) -> Optional[torch.Tensor]:
    """None, 'mean' (1 / number of selected heads) or a float tensor (len(layers), len(heads)) -> None or that float32 tensor (CPU or
    wherever it was).  ValueError on anything else."""
    if head_weights is None:
        return None
    if isinstance(head_weights, str):
        if head_weights != 'mean':
            raise ValueError(f"attention_maps: head_weights must be None, 'mean' or a float tensor, got {head_weights!r}")
        return torch.full((n_layers, n_heads), 1.0 / n_heads, dtype=torch.float32)
    w = torch.as_tensor(head_weights)
    if not w.dtype.is_floating_point or tuple(w.shape) != (n_layers, n_heads):
        raise ValueError(f'attention_maps: head_weights must be a float tensor of shape (len(layers), len(heads)) = ({n_layers}, {n_heads}), '
                         f'got {tuple(w.shape)} {w.dtype}')
    return w.detach().to(torch.float32)


def buffer_bytes(lengths: Sequence[int], n_layers: int, n_out: int, dtype: torch.dtype) -> int:
    """Bytes of the one buffer attention_maps returns views of: L_sel * n_out * sum_b S_b^2 * itemsize."""
    return n_layers * n_out * sum(int(s) * int(s) for s in lengths) * torch.empty(0, dtype=dtype).element_size()


class AttentionMapAccumulator(QKObserver):
    """The observer of attention_maps.  Unselected layers are turned away; the i-th selected layer's maps go to slots i * n_out .. of
    every protein's block run (esme_hip_attn_maps; n_out = len(heads), or 1 with head weights).  layers / heads: validated index lists;
    weights: None or float32 (len(layers), len(heads))."""

    def __init__(self, layers, heads, weights: Optional[torch.Tensor], dtype: torch.dtype, cu_lens: torch.Tensor, max_len: int,
                 model_heads: int, head_pad: int, head_dim: int, keep_qk: bool = False):
        super().__init__(cu_lens, max_len, model_heads, head_pad, head_dim,
                         lambda B, T: _hip_attn_maps.workspace_bytes(B, T, len(heads)), keep_qk)
        dev = cu_lens.device
        self.layers, self.sel = list(layers), list(heads)
        self.slot = {l: i for i, l in enumerate(self.layers)}
        self.head_list = torch.tensor(self.sel, dtype=torch.int32, device=dev)
        self.weights = None if weights is None else weights.to(device=dev, dtype=torch.float32).contiguous()
        self.n_out = 1 if weights is not None else len(self.sel)
        self.S, self.map_off, total = _hip_attn_maps.map_offsets(cu_lens, len(self.layers) * self.n_out)
        self.out = torch.empty(total, dtype=dtype, device=dev)

    def wants(self, index: int) -> bool:
        return index in self.slot

    def launch(self, index: int, q2: torch.Tensor, k2: torch.Tensor, q_prescaled: bool) -> None:
        i = self.slot[index]
        if self.out.numel():
            _hip_attn_maps.attn_maps(q2, k2, self.cu_lens, self.max_len, self.heads, self.head_pad, self.scale, self.head_list, self.out,
                                     self.map_off, i * self.n_out, self.ws, head_weights=None if self.weights is None else self.weights[i],
                                     q_prescaled=q_prescaled)

    def result(self):
        """List of B views of the one buffer: (L_sel, H_sel, S_b, S_b), with head weights (L_sel, S_b, S_b)."""
        if sorted(self.done) != sorted(self.layers):
            raise RuntimeError(f'attention_maps: the forward handed over layers {self.done}, expected {sorted(self.layers)}')
        L = len(self.layers)
        shape = (L,) if self.weights is not None else (L, self.n_out)
        return [self.out[o:o + L * self.n_out * s * s].view(*shape, s, s) for s, o in zip(self.S.tolist(), self.map_off.tolist())]
