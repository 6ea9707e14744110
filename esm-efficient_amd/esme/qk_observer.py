"""The hook through which `predict_contacts`, `contact_features` and `attention_maps` read every layer's final (q, k) in the packed
forward: `ForwardContext.observer` holds a QKObserver, and every attention block calls its `.layer(index, q, k, q_prescaled)`."""
from __future__ import annotations

from typing import Callable

import torch


class QKObserver:
    """Base of the three accumulators.  Owns the batch geometry, the softmax scale, the kernels' workspace and the one `layer()`; a
    subclass holds its output buffer, its kernel call (`launch`) and its `result()`, and may turn layers away (`wants`).
    `workspace_bytes(B, T)`: the subclass's kernel's need.  `keep_qk` (tests): clones of each layer's (layer, q, k, q_prescaled) in `.qk`."""

    def __init__(self, cu_lens: torch.Tensor, max_len: int, heads: int, head_pad: int, head_dim: int,
                 workspace_bytes: Callable[[int, int], int], keep_qk: bool = False):
        self.cu_lens, self.max_len, self.heads, self.head_pad = cu_lens, int(max_len), int(heads), int(head_pad)
        self.scale = float(head_dim) ** -0.5                     # of the LOGICAL head dim (a padded layout's pad lanes are zero)
        B, T = cu_lens.numel() - 1, int(cu_lens[-1])
        self.ws = torch.empty(max(workspace_bytes(B, T), 16), dtype=torch.uint8, device=cu_lens.device)
        self.done = []
        self.qk = [] if keep_qk else None

    def wants(self, index: int) -> bool:
        return True

    def launch(self, index: int, q2: torch.Tensor, k2: torch.Tensor, q_prescaled: bool) -> None:
        """The subclass's kernel call on the (T, H * d) views of one layer it wants (nothing when its output is empty)."""
        raise NotImplementedError

    def layer(self, index: int, q: torch.Tensor, k: torch.Tensor, q_prescaled: bool) -> None:
        wanted = self.wants(index)
        if not wanted and self.qk is None:                       # before any view or clone is made
            return
        T = q.shape[0]
        E = self.heads * self.head_pad
        q2, k2 = (t.view(T, E) if t.dim() == 3 else t for t in (q, k))
        if q2.stride(0) != k2.stride(0) or q2.stride(1) != 1 or k2.stride(1) != 1:
            q2, k2 = q2.contiguous(), k2.contiguous()
        if self.qk is not None:
            self.qk.append((index, q2.clone(), k2.clone(), bool(q_prescaled)))
        if wanted:
            self.launch(index, q2, k2, q_prescaled)
            self.done.append(index)


def dense_blocks(blocks, lead, width: int, dtype: torch.dtype, device) -> torch.Tensor:
    """The per-protein blocks (*lead, n_b, n_b) of a packed result in one zeroed (B, *lead, width, width) tensor, each in its top-left corner."""
    width = max(int(width), 0)
    out = torch.zeros(len(blocks), *lead, width, width, dtype=dtype, device=device)
    for i, m in enumerate(blocks):
        out[i, ..., :m.shape[-2], :m.shape[-1]] = m
    return out
