"""A linear-chain conditional random field over packed per-residue scores: the output layer of signal-peptide and membrane-topology
predictors (SignalP 6.0, DeepTMHMM, TMbed put one on top of a language model's per-residue scores).

`CRF` scores whole label paths: emissions (T, C) plus a learned (C, C) transition matrix, start and end scores, and optional masks
of allowed moves.  Its three methods run on the kernels of include/esme_hip_crf.h through esme.autograd.CRFLogPartition and
esme._hip_crf -- one wavefront per sequence of the `cu_lens`-packed batch, no step per position on the host, no host synchronisation:
 - `loss`: log Z(every residue free) - log Z(labelled residues constrained).  A fully labelled sequence makes the second term the gold
   path's score (the usual CRF negative log-likelihood); an unlabelled residue inside a protein is marginalised over, not skipped.
 - `decode`: the Viterbi path and its score.   - `marginals`: the posterior label probabilities of every residue.
Parameter names and the orientation of `transitions` are pytorch-crf's, so its state dicts load."""
from __future__ import annotations

import torch
from torch import nn

from esme import _hip_crf

FORBIDDEN = -10000.0          # added to the score of a move that `allowed*` forbids (AllenNLP's constant): finite, so nothing is special-cased


def default_chain(cu_lens: torch.Tensor, T: int) -> torch.Tensor:
    """(T,) bool: every row except the first and the last of each sequence -- the residues of a batch whose sequences are framed by
    <cls> and <eos>, as ResidueLabeledDataset's are.  Built on the device from `cu_lens`, without a synchronisation."""
    chain = torch.ones(T, dtype=torch.bool, device=cu_lens.device)
    if T == 0 or cu_lens.numel() < 2:
        return chain
    cu = cu_lens.to(torch.int64)
    # (an empty sequence names the neighbouring sequences' first / last rows, which are excluded already)
    idx = torch.cat((cu[:-1], cu[1:] - 1)).clamp_(0, T - 1)
    return chain.index_fill_(0, idx, False)


class CRF(nn.Module):
    """CRF(num_labels, allowed=None, allowed_start=None, allowed_end=None).

    Parameters (float32, created with requires_grad=False like every head here; opt in with `crf.requires_grad_(True)`):
    `transitions` (C, C) with [i][j] the score of moving from label i to label j, `start_transitions` (C,), `end_transitions` (C,).
    allowed (C, C) / allowed_start (C,) / allowed_end (C,): boolean masks of the moves that may occur (buffers); a forbidden move gets
    -10 000 added to its score.  At most 64 labels.  All methods take packed input: emissions (T, C) and cu_lens (B + 1,)."""

    def __init__(self, num_labels, allowed=None, allowed_start=None, allowed_end=None):
        super().__init__()
        if not 1 <= num_labels <= _hip_crf.MAX_C:
            raise ValueError(f'CRF: num_labels must be in 1 .. {_hip_crf.MAX_C} (one lane of a wavefront per label), got {num_labels}')
        C = self.num_labels = num_labels
        self.transitions = nn.Parameter(torch.empty(C, C, dtype=torch.float32).uniform_(-0.1, 0.1), requires_grad=False)
        self.start_transitions = nn.Parameter(torch.empty(C, dtype=torch.float32).uniform_(-0.1, 0.1), requires_grad=False)
        self.end_transitions = nn.Parameter(torch.empty(C, dtype=torch.float32).uniform_(-0.1, 0.1), requires_grad=False)
        for name, mask, shape in (('allowed', allowed, (C, C)), ('allowed_start', allowed_start, (C,)), ('allowed_end', allowed_end, (C,))):
            mask = torch.ones(shape, dtype=torch.bool) if mask is None else torch.as_tensor(mask).to(torch.bool)
            if tuple(mask.shape) != shape:
                raise ValueError(f'CRF: {name} must have shape {shape}, got {tuple(mask.shape)}')
            self.register_buffer(name, mask.clone())

    def scores(self):
        """(transitions, start, end) as the kernels read them: the parameters with FORBIDDEN added where a move is not allowed, in
        torch ops (the parameters' gradients pass through)."""
        f = lambda p, ok: torch.where(ok, p, p + FORBIDDEN)
        return f(self.transitions, self.allowed), f(self.start_transitions, self.allowed_start), f(self.end_transitions, self.allowed_end)

    def _tags(self, emissions, cu_lens, chain, labels, ignore_index=None):
        if emissions.dim() != 2:
            raise ValueError(f'CRF: emissions must be packed (T, num_labels) rows with cu_lens; got shape {tuple(emissions.shape)} '
                             '(padded (B, S, C) input is not served)')
        T, C = emissions.shape
        if C != self.num_labels:
            raise ValueError(f'CRF: emissions have {C} columns but the CRF has {self.num_labels} labels')
        if cu_lens.dim() != 1 or cu_lens.numel() < 1:
            raise ValueError(f'CRF: cu_lens must be a (B + 1,) tensor, got shape {tuple(cu_lens.shape)}')
        if chain is None:
            chain = default_chain(cu_lens, T)
        elif chain.shape != (T,) or chain.dtype != torch.bool:
            raise ValueError(f'CRF: chain must be a ({T},) bool mask, got shape {tuple(chain.shape)} {chain.dtype}')
        free = torch.where(chain, _hip_crf.FREE, _hip_crf.SKIP).to(torch.int32)
        if labels is None:
            return chain, free, None, None
        if labels.dtype not in (torch.int32, torch.int64):
            raise TypeError(f'CRF: labels must be int32 or int64, got {labels.dtype}')
        if labels.shape != (T,):
            raise ValueError(f'CRF: labels must be ({T},), got {tuple(labels.shape)}')
        labelled = chain & (labels >= 0) & (labels < C)
        if ignore_index is not None:
            labelled = labelled & (labels != ignore_index)
        return chain, free, torch.where(labelled, labels.to(torch.int32), free), labelled

    def log_partition(self, emissions, tags, cu_lens):
        """logz (B,) of esme.autograd.CRFLogPartition on this CRF's scores."""
        from esme.autograd import CRFLogPartition
        A, s, n = self.scores()
        return CRFLogPartition.apply(emissions, A, s, n, tags, cu_lens)

    def loss(self, emissions, labels, cu_lens, chain=None, ignore_index=-100, reduction='mean'):
        """The negative log-likelihood of `labels` as a float32 device scalar with a grad_fn.  chain: (T,) bool, the rows that are
        residues (default: every row but the first and last of each sequence).  Inside the chain a label in [0, C) constrains its row;
        `ignore_index` (also when it lies in [0, C)) and anything else leaves the row free, so it is marginalised over; labels outside the chain are not read.
        reduction: 'sum', 'mean' (over the sequences with a non-empty chain) or 'token_mean' (over the labelled chain rows); a zero
        denominator gives 0."""
        if reduction not in ('sum', 'mean', 'token_mean'):
            raise ValueError(f"CRF.loss: reduction must be 'sum', 'mean' or 'token_mean', got {reduction!r}")
        if labels is None:
            raise ValueError('CRF.loss: labels are required')
        chain, free, tags, labelled = self._tags(emissions, cu_lens, chain, labels, ignore_index)
        nll = self.log_partition(emissions, free, cu_lens) - self.log_partition(emissions, tags, cu_lens)
        total = nll.sum()
        if reduction == 'sum':
            return total
        if reduction == 'token_mean':
            den = labelled.sum()
        else:
            seen = torch.cat((chain.new_zeros(1, dtype=torch.int64), chain.cumsum(0)))
            cu = cu_lens.to(torch.int64).clamp(0, chain.numel())
            den = ((seen[cu[1:]] - seen[cu[:-1]]) > 0).sum()
        return total / den.clamp(min=1).to(torch.float32)

    def decode(self, emissions, cu_lens, chain=None, labels=None, fill=-100):
        """(path (T,) int64, score (B,) float32): the best label of every chain row (`fill` elsewhere) and the best path's score per
        sequence.  labels: constrained decoding -- rows labelled in [0, C) keep their label."""
        from esme.autograd import _f32_rows
        with torch.no_grad():
            _, free, tags, _ = self._tags(emissions, cu_lens, chain, labels)
            A, s, n = (t.contiguous() for t in self.scores())
            return _hip_crf.crf_decode(_f32_rows(emissions), A, s, n, cu_lens.to(torch.int32).contiguous(), free if tags is None else tags,
                                       fill=fill)

    def marginals(self, emissions, cu_lens, chain=None, labels=None):
        """(T, C) float32 posterior label probabilities of the chain rows (zeros elsewhere): the backward with a unit upstream
        gradient."""
        from esme.autograd import _f32_rows
        with torch.no_grad():
            _, free, tags, _ = self._tags(emissions, cu_lens, chain, labels)
            tags = free if tags is None else tags
            A, s, n = (t.contiguous() for t in self.scores())
            e, cu = _f32_rows(emissions), cu_lens.to(torch.int32).contiguous()
            logz, alpha = _hip_crf.crf_fwd(e, A, s, n, cu, tags)
            return _hip_crf.crf_bwd(e, A, s, n, cu, tags, alpha, logz, torch.ones_like(logz), want_params=False)[0]
