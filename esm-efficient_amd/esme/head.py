"""Heads on the HIP path: the LM head (reference esme/head.py:8-27: dense -> GELU -> LN -> vocab)
and the mean-pooling classification head `ClsHead` (esme/head.py:30-68).

The exact-erf GELU is the dense GEMM's epilogue; the vocab projection (N = 33 / 64,
HBM-bound) runs on the same GEMM kernel with row-clamped weight loads.  ClsHead pools
with esme_hip_segment_mean, runs its first Linear on the GEMM and the ReLU + last Linear
in esme_hip_relu_linear (`forward`: inference only; `forward_trainable`: the same function with a backward)."""
from __future__ import annotations

import torch
from torch import nn

from esme import _hip
from esme.nn import Derived, LayerNorm, Linear, pad_last, pad_rows, version_key
from esme.pooling import PartitionMeanPool, _ReluMLP


class RobertaLMHead(nn.Module):
    def __init__(self, embed_dim, vocab_size, dtype=torch.bfloat16, phys_dim=None):
        super().__init__()
        self.embed_dim = embed_dim
        self.phys_dim = phys_dim or embed_dim          # physical (64-aligned) width of the features, see esm.ESM2
        self.dense = Linear(embed_dim, embed_dim, dtype=dtype)
        self.layer_norm = LayerNorm(embed_dim, dtype=dtype)
        self.final = Linear(embed_dim, vocab_size, dtype=dtype)
        self._derived = Derived()

    def _padded_weights(self):
        return self._derived.get('pad', version_key(self.dense.weight, self.dense.bias, self.final.weight), self._build_padded)

    def _build_padded(self):
        Ep = self.phys_dim
        return (pad_rows(pad_last(self.dense.weight.data, Ep), Ep), pad_last(self.dense.bias.data, Ep), pad_last(self.final.weight.data, Ep))

    def forward_exact(self, pair):
        """Split-operand ('exact' / 'half') modes: `pair` (T, 2 E_phys) = [hi | lo] of the final-LayerNorm output -> fp32 logits (T, V)."""
        T, E, Ep = pair.shape[0], self.embed_dim, self.phys_dim
        if pair.shape[1] != 2 * Ep:
            raise ValueError('forward_exact: the pair is (T, 2 * physical width) = [hi | lo]')
        if Ep != E:                                    # padded layout (ESM2-35M): zero-padded weight copies, pad columns stay zero (gelu(0) = 0)
            dw, db, fw = self._padded_weights()
        else:
            dw, db, fw = self.dense.weight, self.dense.bias, self.final.weight
        h = _hip.gemm_fused(pair, dw, db, _hip.EPI_GELU, split_a=True, pair_out=True)
        ln = self.layer_norm
        _hip.layernorm_split(h, ln.weight, ln.bias, ln.eps, E, out=h, in_off=Ep, out_off=Ep)
        y = torch.empty(T, self.final.out_features, dtype=torch.float32, device=pair.device)
        _hip.gemm_fused(h, fw, self.final.bias, split_a=True, out32=y)
        return y

    def forward_trainable(self, x):
        """dense -> GELU -> LayerNorm -> vocabulary projection on (..., E) features in torch ops on the head's own parameters (frozen
        projections of GEMM-tile shape run on the kernel: esme.autograd.frozen_linear), so that mark_lmhead(True) trains it."""
        from esme import autograd as ag
        shape = x.shape
        y = ag.frozen_linear(self.features_trainable(x), self.final)
        return y.view(*shape[:-1], y.shape[-1])

    def features_trainable(self, x):
        """The part of `forward_trainable` before the vocabulary projection: dense -> GELU -> LayerNorm on (..., E) features, as
        (rows, E).  What model.masked_lm_loss hands to the fused projection + cross-entropy instead of materialising the logits."""
        from esme import autograd as ag
        ag.refuse(self.phys_dim != self.embed_dim, 'the padded layout has no backward')
        h = torch.nn.functional.gelu(ag.frozen_linear(x.reshape(-1, x.shape[-1]), self.dense))
        return ag.layer_norm(h, self.layer_norm)

    def forward(self, features):
        shape = features.shape
        x = features.reshape(-1, shape[-1])
        if self.phys_dim == self.embed_dim:
            h = self.dense(x, _hip.EPI_GELU)
            self.layer_norm(h, out=h)
            y = self.final(h)
        else:
            E, Ep = self.embed_dim, self.phys_dim
            if x.shape[1] == E:                        # logical-width features from a caller: pad the columns
                xp = torch.zeros(x.shape[0], Ep, dtype=x.dtype, device=x.device)
                xp[:, :E] = x
                x = xp
            dw, db, fw = self._padded_weights()
            h = _hip.gemm(x, dw, db, _hip.EPI_GELU)    # pad columns: gelu(0) = 0
            self.layer_norm(h[:, :E], out=h[:, :E])
            y = _hip.gemm(h, fw, self.final.bias)
        return y.view(*shape[:-1], y.shape[-1])


class ClsHead(nn.Module):
    """head(mean pool of each sequence's rows).squeeze(-1) (reference esme/head.py:30-68): `forward(x, cu_lens)` -> (n_seq, num_cls),
    or (n_seq,) for one class.  Keys `head.0.*`, `head.2.*`; x bfloat16 or float32 (the output keeps its dtype).  Parameters are
    bfloat16 whatever `dtype` says; fp32 checkpoints cast on load_state_dict."""

    def __init__(self, embed_dim, num_cls=1, hidden_dim=4096, dtype=torch.bfloat16):
        super().__init__()
        if embed_dim % 8 != 0 or hidden_dim % 8 != 0:
            raise ValueError('ClsHead: embed_dim and hidden_dim must be multiples of 8')
        self.pool = PartitionMeanPool()
        self.head = nn.Sequential(
            Linear(embed_dim, hidden_dim, dtype=torch.bfloat16),
            nn.ReLU(),                                 # slot only: the ReLU runs inside esme_hip_relu_linear
            Linear(hidden_dim, num_cls, dtype=torch.bfloat16),
        )
        self._mlp = _ReluMLP()

    def forward(self, x, cu_lens):
        if x.dtype not in (torch.bfloat16, torch.float32):
            raise TypeError(f'ClsHead: x must be bfloat16 or float32, got {x.dtype}')
        pooled = self.pool(x, cu_lens)
        return self._mlp(pooled, self.head[0], self.head[2]).squeeze(-1)

    def forward_trainable(self, x, cu_lens):
        """`forward` with a backward: the same arguments, output shape and dtype, in train() and eval() alike.  The mean pool is the
        kernel (esme.autograd.SegmentMean; its backward spreads dY / length over the sequence's rows, for an x that requires grad), the
        MLP is torch ops (F.linear, relu) on the head's own bfloat16 parameters, which are what is trained.  Parameters are created with
        requires_grad=False; opt in with `head.requires_grad_(True)`."""
        from esme import autograd as ag
        ag.check_head_input(x, [(n, p) for n, p in self.named_parameters()], 'ClsHead')
        pooled = ag.SegmentMean.apply(x, cu_lens)
        return ag.relu_mlp(pooled, self.head[0], self.head[2]).squeeze(-1)


class ResidueHead(nn.Module):
    """A label per residue: one Linear `classifier` over the rows of the representation, the layer Hugging Face's
    EsmForTokenClassification calls by the same name (state-dict keys `classifier.weight`, `classifier.bias`: a head trained there
    loads here).  `forward(x)` -> (..., num_labels) bfloat16 logits on the GEMM kernel and `predict(x)` -> the argmax labels, both
    inference only; `loss(x, labels)` is the training route: esme.loss.linear_cross_entropy on `classifier`, which never forms the
    logits.  At most 64 labels.  Parameters are bfloat16 whatever `dtype` says (fp32 checkpoints cast on load_state_dict) and are
    created with requires_grad=False; opt in with `head.requires_grad_(True)`."""

    def __init__(self, embed_dim, num_labels, dtype=torch.bfloat16):
        super().__init__()
        if embed_dim % 8 != 0:
            raise ValueError('ResidueHead: embed_dim must be a multiple of 8')
        if not 1 <= num_labels <= 64:
            raise ValueError(f'ResidueHead: num_labels must be in 1 .. 64 (the fused loss serves one MFMA column tile), got {num_labels}')
        self.embed_dim, self.num_labels = embed_dim, num_labels
        self.classifier = Linear(embed_dim, num_labels, dtype=torch.bfloat16)

    def forward(self, x):
        if x.dtype != torch.bfloat16:
            raise TypeError(f'ResidueHead: x must be bfloat16, got {x.dtype}')
        with torch.no_grad():
            return self.classifier(x.detach())

    def predict(self, x):
        """(...) int64: the label of the largest logit of every row."""
        return self.forward(x).argmax(dim=-1)

    def loss(self, x, labels, ignore_index=-100, weight=None, reduction='mean'):
        """Cross entropy of classifier(x) against `labels` (...) as a float32 device scalar with a grad_fn: see
        esme.loss.linear_cross_entropy (rows labelled `ignore_index` or outside [0, num_labels) are ignored; no host synchronisation)."""
        from esme.loss import linear_cross_entropy
        return linear_cross_entropy(x, self.classifier, labels, ignore_index=ignore_index, weight=weight, reduction=reduction)


class ResidueCRFHead(nn.Module):
    """A label per residue with a linear-chain CRF on top: `classifier`, the Linear of ResidueHead (the same state-dict keys), gives
    the emissions and `crf` (esme.crf.CRF; keys `crf.transitions`, `crf.start_transitions`, `crf.end_transitions`) scores whole label
    paths -- the output layer of signal-peptide and topology predictors, where independent per-residue softmaxes produce label
    sequences that cannot occur.  `loss(x, labels, cu_lens)` is the training route, `predict(x, cu_lens)` the Viterbi path,
    `marginals(x, cu_lens)` the posterior label probabilities; all take packed rows.  `classifier` is bfloat16, the CRF's parameters
    float32; both are created with requires_grad=False; opt in with `head.requires_grad_(True)`.  **crf_kwargs: CRF's allowed= masks."""

    def __init__(self, embed_dim, num_labels, **crf_kwargs):
        super().__init__()
        from esme.crf import CRF
        if embed_dim % 8 != 0:
            raise ValueError('ResidueCRFHead: embed_dim must be a multiple of 8')
        self.embed_dim, self.num_labels = embed_dim, num_labels
        self.crf = CRF(num_labels, **crf_kwargs)
        self.classifier = Linear(embed_dim, num_labels, dtype=torch.bfloat16)

    def emissions_trainable(self, x):
        """classifier(x) as float32 (T, num_labels) in torch ops on the head's own parameters, with a grad_fn."""
        if x.dtype != torch.bfloat16:
            raise TypeError(f'ResidueCRFHead: x must be bfloat16, got {x.dtype}')
        x = x.reshape(-1, x.shape[-1])
        return torch.nn.functional.linear(x, self.classifier.weight, self.classifier.bias).float()

    def forward(self, x):
        """The emissions without a graph."""
        with torch.no_grad():
            return self.emissions_trainable(x.detach())

    def loss(self, x, labels, cu_lens, chain=None, ignore_index=-100, reduction='mean'):
        """esme.crf.CRF.loss of the emissions: a float32 device scalar with a grad_fn, no host synchronisation."""
        return self.crf.loss(self.emissions_trainable(x), labels, cu_lens, chain=chain, ignore_index=ignore_index, reduction=reduction)

    def predict(self, x, cu_lens, chain=None):
        """(T,) int64: the Viterbi label of every residue, -100 on the rows outside chains."""
        return self.crf.decode(self.forward(x), cu_lens, chain=chain)[0]

    def marginals(self, x, cu_lens, chain=None):
        return self.crf.marginals(self.forward(x), cu_lens, chain=chain)
