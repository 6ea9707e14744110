"""Per-protein pooling of packed residue embeddings.

`partition_mean_pool` / `PartitionMeanPool` keep the reference's names and argument
order (`esme/pooling.py:8-69`): the mean of the rows `cu_lens[i] : cu_lens[i+1]` of a
packed (T, E) embedding for every protein i.  On MI355X it is one segmented-reduction
kernel (`esme_hip_segment_mean`): each protein's rows are read once with 16-byte loads
and accumulated in fp32 -- the reference accumulates in the embedding dtype with
`index_add_`, so for bf16 inputs this path is the more accurate of the two.

The attention-pooling heads keep the reference's names, arguments and state-dict keys
(`AttentionPool`, `LearnedAttentionPool`, `LearnedAggregation`, `BinaryLearnedAggregation`,
esme/pooling.py:72-228).  `forward` is inference only: it detaches its inputs; parameters are
created with requires_grad=False and `dropout_p` must be 0.  `forward_trainable` is the same
function with a backward (opt in with `head.requires_grad_(True)`; see AttentionPool.forward_trainable).  The reference projects every residue with `k` and runs flash
attention on n_cls repeated copies; here the projection is folded into the class-token
queries (`esme_hip_attn_pool_fold`, recomputed on every call) and one kernel reads the
embedding once (`esme_hip_attn_pool`).  Because the queries are fixed, `k.bias` adds a
constant to all scores of a (class token, head) and cancels in the softmax: it does not
change the result (in the reference it moves it only through the bf16 rounding of k).
`embed` may be bf16 ('fast' / 'high' representations) or fp32 ('exact' / 'half'); the
pooled output and everything after it keep that dtype.
"""
from __future__ import annotations

from typing import Tuple

import torch
from torch import nn

from esme import _hip
from esme.nn import Derived, Linear, pad_last, version_key


def partition_mean_pool(embed: torch.Tensor, cu_lens: torch.Tensor) -> torch.Tensor:
    """(B, E) means of the packed rows of `embed` (T, E) bf16 / fp32 on a HIP device."""
    return _hip.segment_mean(embed, cu_lens)


class PartitionMeanPool(nn.Module):
    def forward(self, embed, cu_lens):
        return partition_mean_pool(embed, cu_lens)

    @staticmethod
    def _indices(cu_lens):
        """Protein index of every packed row (reference esme/pooling.py:30-36)."""
        lens = (cu_lens[1:] - cu_lens[:-1]).to(torch.long)
        return torch.repeat_interleave(torch.arange(lens.numel(), device=cu_lens.device), lens)


def _check_dims(attention_heads: int, embed_dim: int, dropout_p: float) -> None:
    if dropout_p != 0.0:
        raise NotImplementedError('attention pooling runs inference only: dropout_p must be 0')
    if attention_heads <= 0 or embed_dim % attention_heads != 0:
        raise ValueError(f'embed_dim {embed_dim} is not a multiple of attention_heads {attention_heads}')
    if embed_dim % 8 != 0:
        raise ValueError(f'embed_dim {embed_dim} must be a multiple of 8')


def _check_embed(embed: torch.Tensor, embed_dim: int) -> None:
    if embed.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f'attention pooling: embed must be bfloat16 or float32, got {embed.dtype}')
    if embed.dim() != 2 or embed.shape[1] != embed_dim:
        raise ValueError(f'attention pooling: embed must be (T, {embed_dim}), got {tuple(embed.shape)}')


def _padded_weight(w, kp):
    return pad_last(w.data, kp).contiguous()


class _ReluMLP:
    """y = final(relu(linear(x))) for the heads: `linear` on the MFMA GEMM (bf16 x: esme_hip_gemm_bf16; fp32 x: the split-operand GEMM
    on the (hi, lo) pair of x with an fp32 result, as RobertaLMHead.forward_exact), then esme_hip_relu_linear.  When the input width is
    not a multiple of 64 (E = 480), x and the weight are zero-padded to the next multiple (the padded weight is cached by version_key)."""

    def __init__(self):
        self._derived = Derived()

    def tensors(self):
        return self._derived.tensors()

    def _weight(self, lin: Linear, kp: int) -> torch.Tensor:
        if kp == lin.in_features:
            return lin.weight
        return self._derived.get('pad', (kp, version_key(lin.weight)), _padded_weight, lin.weight, kp)

    def __call__(self, x: torch.Tensor, lin: Linear, final: Linear) -> torch.Tensor:
        M, K = x.shape
        if M == 0:
            return torch.empty(0, final.out_features, dtype=x.dtype, device=x.device)
        kp = -(-K // 64) * 64
        w = self._weight(lin, kp)
        if kp != K:
            xp = torch.zeros(M, kp, dtype=x.dtype, device=x.device)
            xp[:, :K] = x
            x = xp
        x = x.contiguous()
        if x.dtype == torch.float32:
            pair = torch.empty(M, 2 * kp, dtype=torch.bfloat16, device=x.device)
            _hip.stream_operand(x, pair, None, pair=True)
            h = torch.empty(M, lin.out_features, dtype=torch.float32, device=x.device)
            _hip.gemm_fused(pair, w, lin.bias, split_a=True, out32=h)
        else:
            h = _hip.gemm(x, w, lin.bias)
        return _hip.relu_linear(h, final.weight, final.bias)


class AttentionPool(nn.Module):
    """Attention pooling with given class tokens (reference esme/pooling.py:72-136): `forward(cls, embed, (cu_lens, max_len))` ->
    (n_seq, n_cls, E) in embed's dtype.  Key `k.weight`, `k.bias` (the bias cancels, see the module docstring).  Parameters are
    bfloat16 whatever `dtype` says (the kernels read bf16 weights); fp32 checkpoints cast on load_state_dict."""

    def __init__(self, attention_heads: int, embed_dim: int, dropout_p=0.0, dtype=torch.bfloat16):
        super().__init__()
        _check_dims(attention_heads, embed_dim, dropout_p)
        self.attention_heads = attention_heads
        self.embed_dim = embed_dim
        self.dropout_p = dropout_p
        self.k = Linear(embed_dim, embed_dim, dtype=torch.bfloat16)

    def forward(self, cls: torch.Tensor, embed: torch.Tensor, pad_args: Tuple[torch.Tensor, int]) -> torch.Tensor:
        cu_lens, _max_len = pad_args                   # max_len is not needed (nor trusted)
        _check_embed(embed, self.embed_dim)
        if cls.dim() != 2 or cls.shape[1] != self.embed_dim:
            raise ValueError(f'attention pooling: cls must be (n_cls, {self.embed_dim}), got {tuple(cls.shape)}')
        q = cls.detach()
        if q.dtype != torch.bfloat16 or not q.is_contiguous():
            q = q.to(torch.bfloat16).contiguous()
        U = _hip.attn_pool_fold(q, self.k.weight, self.attention_heads)
        return _hip.attn_pool(embed, cu_lens, U, self.attention_heads, q.shape[0])


    def forward_trainable(self, cls: torch.Tensor, embed: torch.Tensor, pad_args: Tuple[torch.Tensor, int]) -> torch.Tensor:
        """`forward` with a backward: the same arguments, output shape and dtype, in train() and eval() alike.  Differentiable in
        `cls`, `k.weight` and `embed` (bfloat16 or float32), each where it requires grad: the pooling and its backward are the HIP
        kernels (esme.autograd.AttentionPooling), the fold of `k` into `cls` is fp32 torch ops.  Parameters are created with
        requires_grad=False; a user opts in with `head.requires_grad_(True)`.  `k.bias` adds a constant to every score of a (class
        token, head) and cancels in the softmax: its gradient is zero and it is given none (`k.bias.grad is None`).  Embeddings the
        embedding gradient is not wanted for (a frozen backbone: `forward_representation` under no_grad) skip that part of the
        backward kernel.  Parameters must be bfloat16 (NotImplementedError otherwise)."""
        from esme import autograd as ag
        cu_lens, _max_len = pad_args
        _check_embed(embed, self.embed_dim)
        if cls.dim() != 2 or cls.shape[1] != self.embed_dim:
            raise ValueError(f'attention pooling: cls must be (n_cls, {self.embed_dim}), got {tuple(cls.shape)}')
        ag.check_head_input(embed, [('cls', cls), ('k.weight', self.k.weight)], 'attention pooling')
        U = ag.pool_fold(cls, self.k.weight, self.attention_heads)
        return ag.AttentionPooling.apply(embed, cu_lens, U, self.attention_heads, cls.shape[0])


class LearnedAttentionPool(AttentionPool):
    """AttentionPool with `num_cls` learned class tokens, key `cls` (ones at construction, as the reference:
    esme/pooling.py:139-181).  `forward(embed, pad_args)` -> (n_seq, num_cls, E)."""

    def __init__(self, num_cls, attention_heads, embed_dim: int, dropout_p=0.0, dtype=torch.bfloat16):
        super().__init__(attention_heads, embed_dim, dropout_p, dtype)
        self.cls = nn.Parameter(torch.ones(num_cls, embed_dim, dtype=torch.bfloat16), requires_grad=False)

    def forward(self, embed: torch.Tensor, pad_args: Tuple[torch.Tensor, int]) -> torch.Tensor:
        return super().forward(self.cls, embed, pad_args)

    def forward_trainable(self, embed: torch.Tensor, pad_args: Tuple[torch.Tensor, int]) -> torch.Tensor:
        """`forward` with a backward (AttentionPool.forward_trainable) on the learned class tokens."""
        return super().forward_trainable(self.cls, embed, pad_args)


class LearnedAggregation(nn.Module):
    """final(relu(linear(LearnedAttentionPool(embed)))).squeeze(1) (reference esme/pooling.py:184-219): (n_seq, 1) for one class
    token, (n_seq, num_cls, 1) otherwise.  Keys `attn.*`, `linear.*`, `final.*`."""

    def __init__(self, num_cls, attention_heads: int, embed_dim: int, dropout_p=.0, dtype=torch.bfloat16):
        super().__init__()
        self.attn = LearnedAttentionPool(num_cls, attention_heads, embed_dim, dropout_p=dropout_p, dtype=dtype)
        self.linear = Linear(embed_dim, embed_dim, dtype=torch.bfloat16)
        self.relu = nn.ReLU()                          # keeps the reference's module slot; the ReLU runs inside esme_hip_relu_linear
        self.final = Linear(embed_dim, 1, dtype=torch.bfloat16)
        self._mlp = _ReluMLP()

    def forward(self, embed: torch.Tensor, pad_args: Tuple[torch.Tensor, int]) -> torch.Tensor:
        x = self.attn(embed, pad_args)
        n, c, E = x.shape
        y = self._mlp(x.reshape(n * c, E), self.linear, self.final)
        return y.view(n, c, 1).squeeze(1)

    def forward_trainable(self, embed: torch.Tensor, pad_args: Tuple[torch.Tensor, int]) -> torch.Tensor:
        """`forward` with a backward: the pooling as AttentionPool.forward_trainable, the MLP after it in torch ops (F.linear, relu) on
        `linear` and `final`, the weights being trained.  The same output shape and dtype as `forward`, in train() and eval() alike;
        opt in with `head.requires_grad_(True)`; `attn.k.bias` gets no gradient (it is zero)."""
        from esme import autograd as ag
        ag.check_head_input(embed, [(n, p) for n, p in self.named_parameters()], 'LearnedAggregation')
        x = self.attn.forward_trainable(embed, pad_args)
        return ag.relu_mlp(x, self.linear, self.final).squeeze(1)


class BinaryLearnedAggregation(LearnedAggregation):
    """LearnedAggregation with one class token, squeezed to (n_seq,) (reference esme/pooling.py:222-228)."""

    def __init__(self, attention_heads: int, embed_dim: int, dropout_p=0.0, dtype=torch.bfloat16):
        super().__init__(1, attention_heads, embed_dim, dropout_p, dtype)

    def forward(self, embed: torch.Tensor, pad_args: Tuple[torch.Tensor, int]) -> torch.Tensor:
        return super().forward(embed, pad_args).squeeze(-1)

    def forward_trainable(self, embed: torch.Tensor, pad_args: Tuple[torch.Tensor, int]) -> torch.Tensor:
        """`forward` with a backward (LearnedAggregation.forward_trainable), squeezed to (n_seq,)."""
        return super().forward_trainable(embed, pad_args).squeeze(-1)
