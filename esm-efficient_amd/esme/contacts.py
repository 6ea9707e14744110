"""Residue-contact prediction from the attention maps (ESM-2's contact head, Rao et al. 2021), without materialising the maps.

The head is a logistic regression over the symmetrised, APC-corrected attention maps of all layers and heads:
    P = softmax(q k^T * scale) over all S keys,  A = P with the bos / eos rows and columns dropped,  Y = A + A^T,
    N = Y - r r^T / t  (r = row sums of Y, t = their total),  logit = b + sum_{l,h} w[l H + h] N^(l,h),  contact = sigmoid(logit).
The reference package cannot compute it (flash_attn_varlen_func returns no attention weights; its checkpoints drop `contact_head.*`).
Here every layer's attention operands are handed to esme_hip_contact_layer (csrc/contacts.hip), which reduces the layer's H maps
into one (S - 2)^2 fp32 logit map per protein as it computes them: device memory stays at O(H T) plus the output.

ESM-2 publishes its regression weights (`*-contact-regression.pt`: {'model': {'contact_head.regression.weight', ...bias}}).
ESM-C ships none, and neither does a LoRA-adapted or fine-tuned model: fit one with this library.  `model.contact_features` returns
the features N^(l,h)_ij themselves at a list of residue pairs (esme_hip_contact_features: a regression is trained on pairs, not on
maps, so no map is stored here either), `ContactHead.fit` runs the L1-regularised logistic regression of Rao et al. on them, and
`fit_contact_head(model, batches, contact_maps)` does both and returns the head for `model.set_contact_head`.
"""
from __future__ import annotations

import math
import warnings
from typing import Optional

import torch
from torch import nn

from esme import _hip_contact_features, _hip_contacts
from esme.qk_observer import QKObserver


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

    @classmethod
    def fit(cls, X: torch.Tensor, y: torch.Tensor, num_layers: int, attention_heads: int, C: float = 0.15, tol: float = 1e-6,
            max_iter: int = 20000, sample_weight: Optional[torch.Tensor] = None, prepend_bos: bool = True,
            append_eos: bool = True) -> 'ContactHead':
        """L1-regularised logistic regression on the features of `model.contact_features`: X (P, num_layers * attention_heads), y (P)
        labels in [0, 1] (1 = contact), in float64 torch on X's device.  Minimises
            F(w, b) = (1 / P) sum_p s_p logloss(y_p, b + x_p . w) + lam * |w|_1,   lam = 1 / (C P),   s = sample_weight (default: ones).
        C = 0.15 is the value of Rao et al. (2021).  The intercept b is NOT penalised -- liblinear, which the original used through
        scikit-learn, penalises it as one more coefficient; with P in the thousands and lam = 1 / (C P) the difference is far below
        the noise of the labels, and an unpenalised intercept makes the fit invariant to a shift of the features.

        Solver: FISTA with gradient restart on centred, rescaled columns (step from a power iteration); the returned weights are in
        the original feature units.  Contract: on return the KKT residual
            max(|g_b|,  |g_k + lam sign(w_k)| for w_k != 0,  max(|g_k| - lam, 0) for w_k == 0),   g = (1 / P) [X 1]^T (s (sigmoid(z) - y)),
        is at most `tol`; otherwise a UserWarning (ConvergenceWarning: ...) is issued.  `head.fit_info`: 'iterations', 'residual',
        'objective', 'converged', and the float64 solution 'weight' (L H) / 'bias' the residual was taken at (the head stores its
        float32 rounding).  Deterministic: no random numbers, a fixed starting point.  ValueError for P == 0, a wrong width, labels
        outside [0, 1] or of one class only."""
        K = int(num_layers) * int(attention_heads)
        if X.dim() != 2 or X.shape[1] != K:
            raise ValueError(f'ContactHead.fit: X must be (P, {num_layers} * {attention_heads} = {K}), got {tuple(X.shape)}')
        P = X.shape[0]
        if P == 0:
            raise ValueError('ContactHead.fit: no pairs (P == 0)')
        if y.numel() != P:
            raise ValueError(f'ContactHead.fit: {P} rows of features but {y.numel()} labels')
        if not (C > 0 and tol > 0):
            raise ValueError('ContactHead.fit: C and tol must be positive')
        X64 = X.detach().to(torch.float64)
        y64 = y.detach().reshape(-1).to(device=X.device, dtype=torch.float64)
        sw = torch.ones_like(y64) if sample_weight is None else sample_weight.detach().reshape(-1).to(device=X.device, dtype=torch.float64)
        if sw.numel() != P or bool((sw < 0).any()):
            raise ValueError('ContactHead.fit: sample_weight must hold P non-negative values')
        if not bool(torch.isfinite(X64).all()):
            raise ValueError('ContactHead.fit: X holds non-finite values (an out-of-range pair gives a NaN row)')
        if bool(((y64 < 0) | (y64 > 1)).any()):
            raise ValueError('ContactHead.fit: labels must lie in [0, 1]')
        pos, tot = float((sw * y64).sum()), float(sw.sum())
        if not 0.0 < pos < tot:
            raise ValueError('ContactHead.fit: the labels hold one class only; a logistic regression needs contacts and non-contacts')
        lam = 1.0 / (C * P)

        # centred, rescaled columns: x' = (x - mu) / sc, w' = sc * w, b' = b + mu . w; the penalty of w'_k is lam / sc_k
        mu = X64.mean(0)
        sc = (X64 - mu).square().mean(0).sqrt()
        sc = torch.where(sc > 0, sc, torch.ones_like(sc))
        Xs = (X64 - mu) / sc
        lam_s = lam / sc

        def grad(w, b):
            """(g_w', g_b, z) of the smooth part at (w', b')."""
            z = Xs @ w + b
            r = sw * (torch.sigmoid(z) - y64) / P
            return Xs.T @ r, r.sum(), z

        def residual(w, gw, gb):
            g = sc * gw + mu * gb                                # the gradient in the original units, by w = w' / sc
            at = torch.where(w != 0, (g + lam * torch.sign(w)).abs(), (g.abs() - lam).clamp(min=0))
            return float(torch.maximum(at.max() if K else gb.abs(), gb.abs()))

        # Lipschitz constant of the gradient: max(s) / (4 P) * lambda_max([X' 1]^T [X' 1]), by a power iteration from the ones vector
        v, vb = torch.ones(K, dtype=torch.float64, device=X.device), torch.ones((), dtype=torch.float64, device=X.device)
        top = 1.0
        for _ in range(50):
            nrm = torch.sqrt(v.square().sum() + vb * vb)
            v, vb = v / nrm, vb / nrm
            u = Xs @ v + vb
            v, vb = Xs.T @ u, u.sum()
            top = float(torch.sqrt(v.square().sum() + vb * vb))
        lip = 1.1 * float(sw.max()) * top / (4.0 * P)            # (the Rayleigh quotient approaches lambda_max from below: 10 % on top)

        w = torch.zeros(K, dtype=torch.float64, device=X.device)
        b = torch.tensor(math.log(pos / (tot - pos)), dtype=torch.float64, device=X.device)
        vw, vb, t = w.clone(), b.clone(), 1.0
        it, res, check_every = 0, float('inf'), 10
        while it < max_iter:
            gw, gb, _ = grad(vw, vb)
            nw = vw - gw / lip
            nw = torch.sign(nw) * (nw.abs() - lam_s / lip).clamp(min=0)
            nb = vb - gb / lip
            it += 1
            if float((vw - nw) @ (nw - w) + (vb - nb) * (nb - b)) > 0:      # gradient restart (O'Donoghue & Candes): drop the momentum
                t, vw, vb = 1.0, nw, nb
            else:
                t_new = 0.5 * (1.0 + math.sqrt(1.0 + 4.0 * t * t))
                vw, vb = nw + ((t - 1.0) / t_new) * (nw - w), nb + ((t - 1.0) / t_new) * (nb - b)
                t = t_new
            w, b = nw, nb
            if it % check_every == 0 or it == max_iter:
                gw, gb, _ = grad(w, b)
                res = residual(w, gw, gb)
                if res <= tol:
                    break
        w_out = w / sc + 0.0                                     # (+ 0.0: no negative zeros)
        b_out = b - (mu * w_out).sum()
        # the residual and the objective of what is returned, from the original features
        z = X64 @ w_out + b_out
        r = sw * (torch.sigmoid(z) - y64) / P
        g, gb = X64.T @ r, r.sum()
        at = torch.where(w_out != 0, (g + lam * torch.sign(w_out)).abs(), (g.abs() - lam).clamp(min=0))
        res = float(torch.maximum(at.max(), gb.abs()))
        obj = float((sw * (torch.nn.functional.softplus(z) - y64 * z)).sum() / P + lam * w_out.abs().sum())
        if not res <= tol:
            warnings.warn(f'ConvergenceWarning: ContactHead.fit stopped after {it} iterations with a KKT residual of {res:.3e} > tol = {tol:.3e}; '
                          'raise max_iter', UserWarning, stacklevel=2)
        head = cls(num_layers, attention_heads, prepend_bos, append_eos)
        head.regression.weight.data.copy_(w_out.reshape(1, -1).to(torch.float32))
        head.regression.bias.data.copy_(b_out.reshape(1).to(torch.float32))
        head.fit_info = {'iterations': it, 'residual': res, 'objective': obj, 'converged': res <= tol, 'lam': lam,
                         'weight': w_out.clone(), 'bias': float(b_out)}
        return head


class ContactAccumulator(QKObserver):
    """The observer of predict_contacts: adds every layer's share to the packed logit map (esme_hip_contact_layer)."""

    def __init__(self, head: ContactHead, cu_lens: torch.Tensor, max_len: int, heads: int, head_pad: int, head_dim: int, keep_qk: bool = False):
        super().__init__(cu_lens, max_len, heads, head_pad, head_dim, lambda B, T: _hip_contacts.workspace_bytes(B, T, heads), keep_qk)
        dev = cu_lens.device
        self.front, self.back = head.trim
        self.w = head.regression.weight.detach().to(device=dev, dtype=torch.float32).reshape(head.num_layers, heads).contiguous()
        self.bias = float(head.regression.bias.detach().float().reshape(-1)[0])
        self.n, self.map_off, total = _hip_contacts.map_offsets(cu_lens, self.front, self.back)
        self.out = torch.empty(total, dtype=torch.float32, device=dev)

    def launch(self, index: int, q2: torch.Tensor, k2: torch.Tensor, q_prescaled: bool) -> None:
        if self.out.numel():
            _hip_contacts.contact_layer(q2, k2, self.cu_lens, self.max_len, self.heads, self.head_pad, self.scale, self.w[index], self.bias,
                                        not self.done, self.out, self.map_off, self.ws, q_prescaled=q_prescaled,
                                        trim_front=self.front, trim_back=self.back)

    def result(self, num_layers: int, logits: bool):
        if self.done != list(range(num_layers)):
            raise RuntimeError(f'predict_contacts: the forward handed over layers {self.done}, expected 0 .. {num_layers - 1} in order')
        if not logits:
            torch.sigmoid_(self.out)
        n, off = self.n.tolist(), self.map_off.tolist()
        return [self.out[o:o + m * m].view(m, m) for m, o in zip(n, off)]


def all_pairs(n, min_sep: int = 0, device=None) -> torch.Tensor:
    """int32 (P, 3) rows (s, i, j): every i < j with j - i >= min_sep of every sequence, n[s] kept residues each, built on `device`."""
    sep = max(int(min_sep), 1)
    rows = []
    for s, m in enumerate(n):
        if m > sep:
            ij = torch.triu_indices(m, m, offset=sep, device=device)
            rows.append(torch.cat((torch.full((1, ij.shape[1]), s, dtype=ij.dtype, device=device), ij), 0).T)
    if not rows:
        return torch.zeros(0, 3, dtype=torch.int32, device=device)
    return torch.cat(rows, 0).to(torch.int32).contiguous()


def check_pairs(pairs, n, device) -> torch.Tensor:
    """The pair list of `model.contact_features` as a contiguous int32 (P, 3) tensor on `device`: an integer (P, 3) tensor of rows
    (s, i, j), or one integer (P_s, 2) tensor of rows (i, j) per sequence.  ValueError on a row outside its sequence's n[s] kept residues."""
    if isinstance(pairs, (list, tuple)):
        if len(pairs) != len(n):
            raise ValueError(f'contact_features: {len(pairs)} per-sequence pair lists for {len(n)} sequences')
        rows = []
        for s, ij in enumerate(pairs):
            ij = torch.as_tensor(ij)
            if ij.numel() == 0:
                continue
            if ij.dim() != 2 or ij.shape[1] != 2:
                raise ValueError(f'contact_features: sequence {s}: expected a (P_s, 2) tensor of (i, j) rows, got {tuple(ij.shape)}')
            ij = ij.to(device)
            rows.append(torch.cat((torch.full_like(ij[:, :1], s), ij), 1))
        pairs = torch.cat(rows, 0) if rows else torch.zeros(0, 3, dtype=torch.int32)
    pairs = torch.as_tensor(pairs)
    if pairs.dim() != 2 or pairs.shape[1] != 3 or pairs.dtype.is_floating_point or pairs.dtype == torch.bool:
        raise ValueError(f'contact_features: pairs must be an integer (P, 3) tensor of (s, i, j) rows, got {tuple(pairs.shape)} {pairs.dtype}')
    if pairs.shape[0] >= 2 ** 31:
        raise ValueError('contact_features: at most 2^31 - 1 pairs per call')
    wide = pairs.to(device=device, dtype=torch.int64)
    if wide.shape[0]:
        nn_ = torch.tensor(list(n) or [0], dtype=torch.int64, device=device)
        s = wide[:, 0]
        ok = (s >= 0) & (s < len(n))
        lim = nn_[s.clamp(0, max(len(n) - 1, 0))]
        ok &= (wide[:, 1] >= 0) & (wide[:, 1] < lim) & (wide[:, 2] >= 0) & (wide[:, 2] < lim)
        if not bool(ok.all()):
            bad = int((~ok).nonzero()[0])
            raise ValueError(f'contact_features: pair {bad} = (s, i, j) = {tuple(wide[bad].tolist())} is out of range '
                             f'({len(n)} sequences; i, j count the residues without bos / eos)')
    return wide.to(torch.int32).contiguous()


class ContactFeatureAccumulator(QKObserver):
    """The observer of contact_features: every layer's H features of every pair go into columns index * H .. of the (P, L H) float32
    matrix `out` (esme_hip_contact_features).  `pairs`: int32 (P, 3) on the device, already validated."""

    def __init__(self, pairs: torch.Tensor, cu_lens: torch.Tensor, max_len: int, num_layers: int, heads: int, head_pad: int, head_dim: int,
                 trim=(1, 1), keep_qk: bool = False):
        super().__init__(cu_lens, max_len, heads, head_pad, head_dim, lambda B, T: _hip_contact_features.workspace_bytes(B, T, heads), keep_qk)
        self.front, self.back = trim
        self.pairs = pairs
        self.out = torch.empty(pairs.shape[0], int(num_layers) * self.heads, dtype=torch.float32, device=cu_lens.device)

    def launch(self, index: int, q2: torch.Tensor, k2: torch.Tensor, q_prescaled: bool) -> None:
        if self.out.shape[0]:
            _hip_contact_features.contact_features(q2, k2, self.cu_lens, self.max_len, self.heads, self.head_pad, self.scale, self.pairs, self.out,
                                                   index * self.heads, self.ws, q_prescaled=q_prescaled, trim_front=self.front, trim_back=self.back)

    def result(self, num_layers: int) -> torch.Tensor:
        if self.done != list(range(num_layers)):
            raise RuntimeError(f'contact_features: the forward handed over layers {self.done}, expected 0 .. {num_layers - 1} in order')
        return self.out


def fit_contact_head(model, batches, contact_maps, min_sep: int = 6, max_pairs: Optional[int] = None, seed: int = 0, **fit_kw) -> ContactHead:
    """Fit the contact regression of `model` (any family, with or without adapters) on proteins of known structure.

    batches: an iterable of (tokens, pad_args) as `model.contact_features` takes them (pad_args None for 2-D tokens).
    contact_maps: one (n, n) map per protein, in the order the batches hold them, n = the protein's length without bos / eos:
    1 = contact, 0 = no contact, < 0 = no label (unresolved residues; dropped).  Pairs i < j with j - i >= min_sep are used (6 in
    Rao et al.).  max_pairs: keep a uniform sample of that many labelled pairs, drawn with a generator seeded with `seed` (memory
    stays at max_pairs rows plus one batch).  fit_kw goes to ContactHead.fit.  Returns the head, ready for model.set_contact_head."""
    maps = list(contact_maps)
    gen = torch.Generator().manual_seed(int(seed))
    Xs, ys, keys, used = None, None, None, 0
    for tokens, pad_args in batches:
        X, pairs = model.contact_features(tokens, pad_args, min_sep=min_sep)
        B = int(pad_args[0].numel()) - 1 if pad_args is not None else int(tokens.shape[0])
        if used + B > len(maps):
            raise ValueError(f'fit_contact_head: the batches hold more proteins than the {len(maps)} contact maps given')
        s, i, j = (pairs[:, c].long() for c in range(3))
        y = torch.full((pairs.shape[0],), -1.0, dtype=torch.float32, device=X.device)
        for b in range(B):
            m = torch.as_tensor(maps[used + b]).to(device=X.device, dtype=torch.float32)
            sel = (s == b).nonzero().reshape(-1)
            if sel.numel():
                if m.dim() != 2 or int(torch.maximum(i[sel].max(), j[sel].max())) >= min(m.shape):
                    raise ValueError(f'fit_contact_head: contact map {used + b} of shape {tuple(m.shape)} is smaller than its protein')
                y[sel] = m[i[sel], j[sel]]
        used += B
        keep = ((y >= 0) & ((j - i).abs() >= min_sep)).nonzero().reshape(-1)
        X, y = X[keep], y[keep]
        key = torch.rand(keep.numel(), generator=gen, dtype=torch.float64).to(X.device)     # (drawn whether or not max_pairs is set)
        Xs, ys, keys = (X, y, key) if Xs is None else (torch.cat((Xs, X)), torch.cat((ys, y)), torch.cat((keys, key)))
        if max_pairs is not None and keys.numel() > max_pairs:                              # the max_pairs smallest keys: a uniform sample
            top = torch.sort(keys, stable=True).indices[:max_pairs].sort().values
            Xs, ys, keys = Xs[top], ys[top], keys[top]
    if used != len(maps):
        raise ValueError(f'fit_contact_head: {len(maps)} contact maps for {used} proteins')
    if Xs is None:
        raise ValueError('fit_contact_head: no batches')
    return ContactHead.fit(Xs, ys, len(model.layers), model.attention_heads, **fit_kw)
