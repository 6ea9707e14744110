"""Residue-contact prediction from the attention maps (ESM-2's contact head, Rao et al. 2021), without materialising the maps.

The head is a logistic regression over the symmetrised, APC-corrected attention maps of all layers and heads:
    P = softmax(q k^T * scale) over all S keys,  A = P with the bos / eos rows and columns dropped,  Y = A + A^T,
    N = Y - r r^T / t  (r = row sums of Y, t = their total),  logit = b + sum_{l,h} w[l H + h] N^(l,h),  contact = sigmoid(logit).
The reference package cannot compute it (flash_attn_varlen_func returns no attention weights; its checkpoints drop `contact_head.*`).
Here every layer's attention operands are handed to esme_hip_contact_layer (csrc/contacts.hip), which reduces the layer's H maps
into one (S - 2)^2 fp32 logit map per protein as it computes them: device memory stays at O(H T) plus the output.

ESM-2 publishes its regression weights (`*-contact-regression.pt`: {'model': {'contact_head.regression.weight', ...bias}}).
ESM-C ships none: train your own logistic regression on the same features and load it with `ContactHead.load`.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from esme import _hip, _hip_contacts


class ContactHead(nn.Module):
    """The regression of the contact head: `regression` = nn.Linear(num_layers * attention_heads, 1) in float32, features in
    layer-major order (l * H + h); `prepend_bos` / `append_eos`: the rows dropped at either end of every sequence."""

    def __init__(self, num_layers: int, attention_heads: int, prepend_bos: bool = True, append_eos: bool = True):
        super().__init__()
        self.num_layers, self.attention_heads = int(num_layers), int(attention_heads)
        self.prepend_bos, self.append_eos = bool(prepend_bos), bool(append_eos)
        self.regression = nn.Linear(self.num_layers * self.attention_heads, 1, dtype=torch.float32)
        for p in self.parameters():
            p.requires_grad_(False)

    @property
    def trim(self):
        return int(self.prepend_bos), int(self.append_eos)

    @staticmethod
    def _regression_tensors(state):
        if isinstance(state.get('model'), dict):               # the published *-contact-regression.pt layout
            state = state['model']
        w = [v for k, v in state.items() if k.endswith('regression.weight')]
        b = [v for k, v in state.items() if k.endswith('regression.bias')]
        if len(w) != 1 or len(b) != 1:
            raise ValueError("ContactHead.load: expected exactly one '...regression.weight' and one '...regression.bias' entry, "
                             f'found {len(w)} / {len(b)}')
        return w[0], b[0]

    @classmethod
    def load(cls, source, num_layers: Optional[int] = None, attention_heads: Optional[int] = None, prepend_bos: bool = True,
             append_eos: bool = True) -> 'ContactHead':
        """From a safetensors file, a torch.load(weights_only=True) file or a state dict: the entries ending in `regression.weight` /
        `regression.bias` (also inside a top-level 'model' dict).  Give num_layers and attention_heads to have the width checked
        (ValueError when num_layers * attention_heads differs); without them the head is one 'layer' of that many features, and
        `model.set_contact_head` re-shapes it to the model."""
        if isinstance(source, dict):
            state = source
        else:
            path = str(source)
            if path.endswith('.safetensors'):
                from safetensors.torch import load_file
                state = load_file(path)
            else:
                state = torch.load(path, map_location='cpu', weights_only=True)
        w, b = cls._regression_tensors(state)
        w, b = w.detach().to(torch.float32).reshape(1, -1), b.detach().to(torch.float32).reshape(1)
        n = w.shape[1]
        if num_layers is None or attention_heads is None:
            num_layers, attention_heads = 1, n
        if num_layers * attention_heads != n:
            raise ValueError(f'ContactHead.load: the regression has {n} features, but num_layers * attention_heads = '
                             f'{num_layers} * {attention_heads} = {num_layers * attention_heads}')
        head = cls(num_layers, attention_heads, prepend_bos, append_eos)
        head.regression.weight.data.copy_(w)
        head.regression.bias.data.copy_(b)
        return head


class ContactAccumulator:
    """What ForwardContext.contacts holds during predict_contacts: every attention block hands it its final (q, k) and it adds that
    layer's share to the packed logit map.  `keep_qk` (tests): clones of each layer's (layer, q, k, q_prescaled) in `.qk`."""

    def __init__(self, head: ContactHead, cu_lens: torch.Tensor, max_len: int, heads: int, head_pad: int, head_dim: int, keep_qk: bool = False):
        dev = cu_lens.device
        self.cu_lens, self.max_len, self.heads, self.head_pad = cu_lens, int(max_len), int(heads), int(head_pad)
        self.scale = float(head_dim) ** -0.5                     # of the LOGICAL head dim (a padded layout's pad lanes are zero)
        self.front, self.back = head.trim
        self.w = head.regression.weight.detach().to(device=dev, dtype=torch.float32).reshape(head.num_layers, heads).contiguous()
        self.bias = float(head.regression.bias.detach().float().reshape(-1)[0])
        self.n, self.map_off, total = _hip_contacts.map_offsets(cu_lens, self.front, self.back)
        self.out = torch.empty(total, dtype=torch.float32, device=dev)
        B, T = cu_lens.numel() - 1, int(cu_lens[-1])
        self.ws = torch.empty(max(_hip_contacts.workspace_bytes(B, T, heads), 16), dtype=torch.uint8, device=dev)
        self.done = []
        self.qk = [] if keep_qk else None

    def layer(self, index: int, q: torch.Tensor, k: torch.Tensor, q_prescaled: bool) -> None:
        T = q.shape[0]
        E = self.heads * self.head_pad
        q2, k2 = (t.view(T, E) if t.dim() == 3 else t for t in (q, k))
        if q2.stride(0) != k2.stride(0) or q2.stride(1) != 1 or k2.stride(1) != 1:
            q2, k2 = q2.contiguous(), k2.contiguous()
        if self.qk is not None:
            self.qk.append((index, q2.clone(), k2.clone(), bool(q_prescaled)))
        if self.out.numel():
            _hip_contacts.contact_layer(q2, k2, self.cu_lens, self.max_len, self.heads, self.head_pad, self.scale, self.w[index], self.bias,
                                        not self.done, self.out, self.map_off, self.ws, q_prescaled=q_prescaled,
                                        trim_front=self.front, trim_back=self.back)
        self.done.append(index)

    def result(self, num_layers: int, logits: bool):
        if self.done != list(range(num_layers)):
            raise RuntimeError(f'predict_contacts: the forward handed over layers {self.done}, expected 0 .. {num_layers - 1} in order')
        if not logits:
            torch.sigmoid_(self.out)
        n, off = self.n.tolist(), self.map_off.tolist()
        return [self.out[o:o + m * m].view(m, m) for m, o in zip(n, off)]
