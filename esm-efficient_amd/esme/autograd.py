"""The autograd seam of LoRA fine-tuning: the two nodes whose forward AND backward are this package's kernels.

 - `VarlenAttention`: forward = esme_hip_attn_varlen_fwd on the current stream (the plain form: q not prescaled, bf16), backward =
   esme_hip_attn_varlen_bwd (include/esme_hip_attn_bwd.h).  torch has no stand-in for the backward of block-diagonal attention over a
   cu_lens-packed batch; everything else of a training step is torch.autograd on torch ops.
 - `FrozenLinear`: a projection whose weight does not require grad: forward = the GEMM kernel, backward dX = dY W on the same kernel
   against W^T from the derived-weight cache (esme.nn.weight_t).  No weight gradient exists for any big GEMM.

`forward_trainable` of the attention block, the layer and the model (esme/attention.py, esme/esm.py) is written with these two and
torch ops, in the reference's unfused data flow.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from esme import _hip, _hip_attn_bwd
from esme.nn import weight_t


class VarlenAttention(torch.autograd.Function):
    """out (T, H * d) = varlen attention of q, k, v (T, H * d) bfloat16 over the sequences of `cu_lens`."""

    @staticmethod
    def forward(ctx, q, k, v, cu_lens, max_len, heads, softmax_scale):
        T, E = q.shape
        qkv = torch.empty(T, 3 * E, dtype=torch.bfloat16, device=q.device)       # (one row stride: the layout both kernels read)
        for i, t in enumerate((q, k, v)):
            qkv[:, i * E:(i + 1) * E].copy_(t)
        q, k, v = (qkv[:, i * E:(i + 1) * E] for i in range(3))
        if cu_lens.dtype != torch.int32:
            cu_lens = cu_lens.to(torch.int32)
        o = _hip.attn_varlen(q, k, v, cu_lens, int(max_len), int(heads), softmax_scale=float(softmax_scale))
        ctx.save_for_backward(qkv, o, cu_lens)
        ctx.args = (int(max_len), int(heads), float(softmax_scale))
        return o

    @staticmethod
    def backward(ctx, d_o):
        qkv, o, cu_lens = ctx.saved_tensors
        E = o.shape[1]
        if d_o.stride(1) != 1 or d_o.stride(0) % 8 or d_o.data_ptr() % 16:
            d_o = d_o.contiguous()
        max_len, heads, scale = ctx.args
        dq, dk, dv = _hip_attn_bwd.attn_varlen_bwd(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], o, d_o, cu_lens, max_len, heads, scale)
        return dq, dk, dv, None, None, None, None


class FrozenLinear(torch.autograd.Function):
    """y = x W^T + b on the GEMM kernel for a W that takes no gradient; dX = dY W on the same kernel (`wt` = W^T, contiguous)."""

    @staticmethod
    def forward(ctx, x, w, b, wt):
        ctx.wt = wt
        return _hip.gemm(x if x.stride(-1) == 1 else x.contiguous(), w, b)

    @staticmethod
    def backward(ctx, dy):
        if dy.stride(1) != 1 or dy.stride(0) % 8 or dy.data_ptr() % 16:
            dy = dy.contiguous()
        return _hip.gemm(dy, ctx.wt), None, None, None


def frozen_linear(x: torch.Tensor, lin) -> torch.Tensor:
    """lin(x) for a 2-D bfloat16 x, differentiable in x (and in lin's parameters where they require grad).  The kernels serve a frozen
    bfloat16 projection whose two widths are multiples of the GEMM's K tile of 64; a trainable one (mark_lmhead) or another shape (the
    vocabulary projection: dX = dY W has K = vocab_size) is torch's F.linear."""
    w, b = lin.weight, lin.bias
    trainable = w.requires_grad or (b is not None and b.requires_grad)
    if trainable or w.shape[0] % 64 or w.shape[1] % 64:
        return F.linear(x, w, b)
    return FrozenLinear.apply(x, w, b, weight_t(lin))


def lora_linear(x: torch.Tensor, mod, names) -> torch.Tensor:
    """The projection `mod` (an esme.nn.Linear, or an esme.lora.LoRA around one) with the adapters `names` selects:
    base(x) + sum_n scaling * (x A_n^T) B_n^T, the delta in torch ops (the gradients of A_n and B_n are torch's)."""
    from esme.lora import LoRA
    if not isinstance(mod, LoRA):
        return frozen_linear(x, mod)
    y = frozen_linear(x, mod.layer)
    for n in mod.select(names):
        y = y + F.linear(F.linear(x, mod.lora_A[n]), mod.lora_B[n]) * mod.scaling
    return y


def layer_norm(x: torch.Tensor, ln) -> torch.Tensor:
    return F.layer_norm(x, (x.shape[-1],), ln.weight, ln.bias, ln.eps)


def rotate_half(x: torch.Tensor) -> torch.Tensor:
    x1, x2 = x.chunk(2, dim=-1)
    return torch.cat((-x2, x1), dim=-1)


def rotary(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, heads: int) -> torch.Tensor:
    """x (T, H * d) rotated with the tables (max_len, d) at the rows' positions, in torch ops: autograd's backward is the inverse
    rotation (the reference's hand-written backward applies the forward rotation again: DESIGN.md section 8)."""
    T, E = x.shape
    x3 = x.view(T, heads, E // heads)
    c, s = cos[pos].unsqueeze(1), sin[pos].unsqueeze(1)
    return (x3 * c + rotate_half(x3) * s).reshape(T, E)


def pad_rows(x: torch.Tensor, indices: torch.Tensor, batch: int, seqlen: int) -> torch.Tensor:
    """`pad_input` in torch ops: packed rows scattered into zeros, (B, S, C)."""
    out = torch.zeros(batch * seqlen, x.shape[-1], dtype=x.dtype, device=x.device)
    return out.index_copy(0, indices.to(torch.int64), x).view(batch, seqlen, x.shape[-1])


def refuse(cond: bool, what: str) -> None:
    if cond:
        raise NotImplementedError(f'forward_trainable: {what}')


def check_linear(lin, what: str) -> None:
    """Quantised storage has no backward here: name it."""
    refuse(lin.weight.dtype != torch.bfloat16, f'{what} is stored quantised ({lin.weight.dtype}); training needs unquantised bfloat16 base weights')
