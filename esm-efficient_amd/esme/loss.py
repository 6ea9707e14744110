"""Masked-token losses with the reference's signatures and semantics (its esme/loss.py): the rows `mask` selects, the padding token
ignored, everything else handed to torch's loss (`*_kwargs`)."""
import torch.nn.functional as F

from esme.alphabet import Alphabet3


def nll_loss(log_probs, tokens, mask, nll_loss_kwargs=None, alphabet=Alphabet3):
    """Negative log likelihood of the target `tokens` at the positions where `mask` is True; `log_probs` (..., V) as
    model.predict_log_prob returns them."""
    log_probs = log_probs.reshape(-1, log_probs.size(-1))
    mask = mask.reshape(-1)
    return F.nll_loss(log_probs[mask], tokens.reshape(-1)[mask], ignore_index=alphabet.padding_idx, **(nll_loss_kwargs or {}))


def cross_entropy(logits, tokens, mask, cross_entropy_loss_kwargs=None, alphabet=Alphabet3):
    """Cross entropy of the target `tokens` at the positions where `mask` is True; `logits` (..., V) as model(...) or
    model.forward_trainable(...) returns them."""
    logits = logits.reshape(-1, logits.size(-1))
    mask = mask.reshape(-1)
    return F.cross_entropy(logits[mask], tokens.reshape(-1)[mask], ignore_index=alphabet.padding_idx, **(cross_entropy_loss_kwargs or {}))


def linear_cross_entropy(x, lin, labels, ignore_index=-100, weight=None, reduction='mean'):
    """Cross entropy of the logits `lin(x)` against `labels` without materialising the logits and without a host synchronisation
    (esme.autograd.LinearCrossEntropy, include/esme_hip_linear_xent.h): a float32 device scalar, differentiable in x and in lin's
    parameters where they require grad.

    x (..., E) bfloat16 and labels (...) int32 / int64 are flattened to rows; lin is an esme.nn.Linear of at most 64 outputs.  A row
    whose label is `ignore_index`, negative or >= C is ignored (torch raises a device assert on an out-of-range label; here it never
    indexes anything).  weight: per-class weights (C,), used in float32.  reduction: 'sum', or 'mean' = torch's weighted mean, the sum
    divided by the kept rows' weights -- except that a batch with nothing kept gives 0 with zero gradients where torch gives NaN:
    nothing on the host can look at the count without a synchronisation, and a NaN would reach the optimiser's master weights."""
    import torch
    from esme import autograd as ag
    if reduction not in ('mean', 'sum'):
        raise ValueError(f"linear_cross_entropy: reduction must be 'mean' or 'sum', got {reduction!r}")
    ag.refuse(ag._is_quantised(lin), 'linear_cross_entropy: a quantised projection has no fused loss (keep the head in bfloat16)')
    w, b = lin.weight, lin.bias
    ag.refuse(w.dtype != torch.bfloat16 or (b is not None and b.dtype != torch.bfloat16),
              f'linear_cross_entropy: the projection must be bfloat16, got {w.dtype}')
    ag.refuse(x.dtype != torch.bfloat16, f'linear_cross_entropy: x must be bfloat16, got {x.dtype} (precisions \'exact\' / \'half\' hand out '
              'float32 representations, which the fused loss does not take)')
    C, E = w.shape
    ag.refuse(C > 64, f'linear_cross_entropy: {C} classes; the fused loss serves at most 64 (one MFMA column tile)')
    ag.refuse(E != lin.in_features or C != lin.out_features or E % 8 != 0,
              f'linear_cross_entropy: a padded projection ({tuple(w.shape)} stored for {lin.in_features} -> {lin.out_features}) or a width '
              'that is no multiple of 8 has no fused loss')
    if x.dim() < 1 or x.shape[-1] != E:
        raise ValueError(f'linear_cross_entropy: x has {tuple(x.shape)} but the projection takes {E} features')
    if tuple(labels.shape) != tuple(x.shape[:-1]):
        raise ValueError(f'linear_cross_entropy: labels {tuple(labels.shape)} do not match the rows of x {tuple(x.shape[:-1])}')
    if labels.dtype not in (torch.int32, torch.int64):
        raise TypeError(f'linear_cross_entropy: labels must be int32 or int64, got {labels.dtype}')
    if weight is not None:
        if tuple(weight.shape) != (C,):
            raise ValueError(f'linear_cross_entropy: weight {tuple(weight.shape)} must be ({C},)')
        weight = weight.detach().to(device=x.device, dtype=torch.float32).contiguous()
    return ag.LinearCrossEntropy.apply(x.reshape(-1, E), w, b, labels.reshape(-1), int(ignore_index), weight, reduction == 'mean')
