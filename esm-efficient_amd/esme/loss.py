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
