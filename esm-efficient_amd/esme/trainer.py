"""Supervised fine-tuning: a backbone, a task head and the layers the head is fed from, as one plain nn.Module.

`RegressionModel` mirrors the forward of the reference's `RegressionTrainer` (esme/trainer.py:47-104) without Lightning: the
representation of the backbone -- the final-LayerNorm output, with `layers=[...]` followed by the raw outputs of those layers on the
feature axis -- goes to the head, whole (`reduction=None`: the head receives `(embed, pad_args)`) or reduced over dim 1 of the padded
output.  `forward` is the inference route (model.forward_representation and the head's fused `forward`, under no_grad);
`forward_trainable` is the same function with a backward (model.forward_trainable(logits=False, layers=...) and the head's
`forward_trainable`).  The training loop is the caller's: see tools/regression_finetune.py.  `ResidueModel` is the per-residue
counterpart: a backbone and a ResidueHead, whose loss is the fused projection + cross-entropy kernel (tools/residue_finetune.py).
The Lightning modules stay out of scope."""
from __future__ import annotations

import torch
from torch import nn


class RegressionModel(nn.Module):
    """RegressionModel(model, head, layers=None, reduction=None).

    model: an esme.ESM2 / ESMC (frozen, with LoRA adapters, or with mark_trainable() layers).  head: a task head whose input width
    is `model.embed_dim * (1 + len(layers))` -- BinaryLearnedAggregation / LearnedAggregation (called with `(embed, pad_args)`),
    ClsHead (called with `(embed, cu_lens)`), or with a reduction any module over (B, width).  layers: the layers to tap, as
    forward_representation(layers=) takes them.  reduction: None, or 'mean' / 'sum' over dim 1 of the PADDED output (call with
    pad_output=True or 2-D tokens), pad rows included, as the reference does."""

    def __init__(self, model, head, layers=None, reduction=None):
        super().__init__()
        if reduction not in (None, 'mean', 'sum'):
            raise ValueError(f"Unknown reduction: {reduction}, expected `'mean'`, `'sum'` or `None`")
        self.plm, self.head = model, head
        self.layers = list(layers) if layers else None
        self.reduction = reduction
        if self.layers:
            model._check_layers_arg(self.layers)

    @property
    def width(self) -> int:
        """The head's input width: embed_dim * (1 + number of tapped layers)."""
        return self.plm.embed_dim * (1 + len(self.layers or ()))

    def reduce(self, x):
        if x.dim() != 3:
            raise ValueError(f'reduction {self.reduction!r} runs over dim 1 of the padded (B, S, width) output; got shape {tuple(x.shape)} '
                             '(pass pad_output=True or 2-D tokens)')
        return x.mean(dim=1) if self.reduction == 'mean' else x.sum(dim=1)

    def _head(self, embed, pad_args, trainable):
        from esme.head import ClsHead
        call = getattr(self.head, 'forward_trainable', self.head) if trainable else self.head
        if self.reduction is not None:
            return call(self.reduce(embed))
        if isinstance(self.head, ClsHead):
            return call(embed, pad_args[0])
        return call(embed, pad_args)

    def forward(self, token, pad_args=None, pad_output=False, pad_indices=None, lora_names=None):
        """Predictions without a graph: forward_representation (the fused inference forward) -> head."""
        with torch.no_grad():
            embed = self.plm.forward_representation(token, pad_args, pad_output=pad_output, pad_indices=pad_indices, lora_names=lora_names,
                                                    layers=self.layers)
            return self._head(embed, pad_args, False)

    def backbone_trains(self) -> bool:
        return any(p.requires_grad for p in self.plm.parameters())

    def forward_trainable(self, token, pad_args=None, pad_output=False, pad_indices=None, lora_names=None, checkpoint_layers=False):
        """The same predictions with a grad_fn: differentiable in the head's parameters and in whatever the backbone trains (adapters,
        mark_trainable() layers) through model.forward_trainable(logits=False, layers=...).  A backbone none of whose parameters
        requires grad is run through forward_representation under no_grad instead (the fused forward: only the head trains)."""
        if self.backbone_trains():
            embed = self.plm.forward_trainable(token, pad_args, pad_output=pad_output, pad_indices=pad_indices, lora_names=lora_names,
                                               logits=False, checkpoint_layers=checkpoint_layers, layers=self.layers)
        else:
            with torch.no_grad():
                embed = self.plm.forward_representation(token, pad_args, pad_output=pad_output, pad_indices=pad_indices,
                                                        lora_names=lora_names, layers=self.layers)
        return self._head(embed, pad_args, True)

    def param_groups(self, lr=1e-5, lr_head=1e-4):
        """The reference's two learning-rate groups, for esme.optim.AdamW: the head's parameters at `lr_head`, the backbone's at `lr`
        (its defaults are the reference's).  Only parameters that require grad are listed; a group that would be empty is left out."""
        groups = [{'params': [p for p in self.head.parameters() if p.requires_grad], 'lr': lr_head},
                  {'params': [p for p in self.plm.parameters() if p.requires_grad], 'lr': lr}]
        return [g for g in groups if g['params']]


def spearman(x: torch.Tensor, y: torch.Tensor) -> float:
    """Spearman's rank correlation of two 1-D tensors (average ranks for ties), in float64 torch ops."""
    def ranks(v):
        v = v.detach().double().flatten().cpu()
        order = torch.argsort(v, stable=True)
        r = torch.empty_like(v)
        r[order] = torch.arange(1, v.numel() + 1, dtype=torch.float64)
        _, inv, counts = torch.unique(v, return_inverse=True, return_counts=True)
        sums = torch.zeros(counts.numel(), dtype=torch.float64).index_add_(0, inv, r)
        return (sums / counts)[inv]
    a, b = ranks(x), ranks(y)
    if a.numel() < 2:
        return float('nan')
    a, b = a - a.mean(), b - b.mean()
    den = float(a.norm() * b.norm())
    return float(a @ b) / den if den > 0 else float('nan')


class ResidueModel(nn.Module):
    """ResidueModel(model, head, layers=None): a backbone and an esme.head.ResidueHead for a label per residue (secondary structure,
    binding sites, disorder, ...), the packed counterpart of Hugging Face's EsmForTokenClassification.

    model: an esme.ESM2 / ESMC (frozen, with LoRA adapters, or with mark_trainable() layers).  head: a ResidueHead of input width
    `model.embed_dim * (1 + len(layers))`.  layers: the layers to tap, as forward_representation(layers=) takes them.  `forward` is the
    inference route (logits under no_grad); `loss_trainable` is the training step's loss, a float32 device scalar whose forward and
    backward never synchronise with the host (esme.loss.linear_cross_entropy).  The training loop is the caller's: see
    tools/residue_finetune.py."""

    def __init__(self, model, head, layers=None):
        super().__init__()
        self.plm, self.head = model, head
        self.layers = list(layers) if layers else None
        if self.layers:
            model._check_layers_arg(self.layers)
        if getattr(head, 'embed_dim', self.width) != self.width:
            raise ValueError(f'ResidueModel: the head takes {head.embed_dim} features but the representation has {self.width} '
                             f'(embed_dim {model.embed_dim} x (1 + {len(self.layers or ())} tapped layers))')

    @property
    def width(self) -> int:
        """The head's input width: embed_dim * (1 + number of tapped layers)."""
        return self.plm.embed_dim * (1 + len(self.layers or ()))

    def forward(self, token, pad_args=None, pad_output=False, pad_indices=None, lora_names=None):
        """Logits (T, C) / (B, S, C) without a graph: forward_representation (the fused inference forward) -> head."""
        with torch.no_grad():
            embed = self.plm.forward_representation(token, pad_args, pad_output=pad_output, pad_indices=pad_indices, lora_names=lora_names,
                                                    layers=self.layers)
            return self.head(embed)

    def predict(self, token, pad_args=None, lora_names=None):
        """The argmax label of every row; with a CRF head (esme.head.ResidueCRFHead) the Viterbi path, -100 outside the chains."""
        if hasattr(self.head, 'crf'):
            with torch.no_grad():
                embed = self.plm.forward_representation(token, pad_args, lora_names=lora_names, layers=self.layers)
                return self.head.predict(embed, pad_args[0])
        return self.forward(token, pad_args, lora_names=lora_names).argmax(dim=-1)

    def backbone_trains(self) -> bool:
        return any(p.requires_grad for p in self.plm.parameters())

    def representation_trainable(self, token, pad_args=None, lora_names=None, checkpoint_layers=False):
        """What the head's loss reads: model.forward_trainable(logits=False, layers=...), or, for a backbone none of whose parameters
        requires grad, forward_representation under no_grad (the fused forward: only the head trains; a frozen backbone that carries
        adapters has to be in eval() for it, as for any inference call)."""
        if self.backbone_trains():
            return self.plm.forward_trainable(token, pad_args, lora_names=lora_names, logits=False, checkpoint_layers=checkpoint_layers,
                                              layers=self.layers)
        with torch.no_grad():
            return self.plm.forward_representation(token, pad_args, lora_names=lora_names, layers=self.layers)

    def loss_trainable(self, token, pad_args, label, lora_names=None, checkpoint_layers=False, weight=None, reduction='mean',
                       ignore_index=-100):
        """The cross entropy of the head's logits against `label` (aligned with `token`: ResidueLabeledDataset's `label`), differentiable
        in the head's parameters and in whatever the backbone trains."""
        embed = self.representation_trainable(token, pad_args, lora_names=lora_names, checkpoint_layers=checkpoint_layers)
        if hasattr(self.head, 'crf'):                             # a CRF head scores label paths: it needs the sequences (`weight` does not apply)
            if weight is not None:
                raise ValueError('ResidueModel: class weights do not apply to a CRF head')
            return self.head.loss(embed, label, pad_args[0], ignore_index=ignore_index, reduction=reduction)
        return self.head.loss(embed, label, ignore_index=ignore_index, weight=weight, reduction=reduction)

    def param_groups(self, lr=1e-5, lr_head=1e-4):
        """Two learning-rate groups for esme.optim.AdamW, as RegressionModel.param_groups: the head's parameters at `lr_head`, the
        backbone's at `lr`.  Only parameters that require grad are listed; a group that would be empty is left out."""
        groups = [{'params': [p for p in self.head.parameters() if p.requires_grad], 'lr': lr_head},
                  {'params': [p for p in self.plm.parameters() if p.requires_grad], 'lr': lr}]
        return [g for g in groups if g['params']]
