"""float64 reference, per-element error bound and CPU emulation for esme_hip_contact_features (csrc/contacts.hip,
include/esme_hip_contact_features.h): the contact regression's features at chosen residue pairs.

`reference_features` restates the definition in float64 on the operands the kernel was handed: per layer l and head h, with P, A, Y, r, t
as in tests/contact_bounds.py,  X[p, l H + h] = N^(l,h)_ij = Y_ij - r_i r_j / t  for pair p = (s, i, j), i and j counted from the first
kept row of sequence s.  `feature_bound` is the sum of the rounding steps behind one such value, each tagged with the marker of the
kernel line that performs it; the statistics m, l, r, t come from the three kernels esme_hip_contact_layer runs too, so their terms are
the ones of contact_bounds.contact_bound, restated here because that function keeps them to itself.  Nothing is tuned to a GPU run.

The two scores of a pair are NOT formed on the MFMA: contact_gather_kernel multiplies eight bf16 elements per lane (exact products in
fp32) into a serial fused-multiply-add chain (7 rounded additions, [dot]) and joins the d / 8 lanes of a head in a butterfly
(log2(d / 8) rounded additions, [dot-tree]).  Its term is therefore the WORST-CASE one, (7 + log2(d / 8)) * 2^-24 * sum_c |q_c k_c|,
not the statistical C_DOT form the MFMA passes use.

`emulate_features` is a float32 CPU emulation of the data flow with switches for defects; tests/test_contact_features_cpu.py checks that
the bound accepts the correct emulation and rejects each defect.  `make_pairs` builds the pair list both test files use.
"""
import math

import torch

from contact_bounds import LN2, LOG2E, TILE, _lens, _scores2, make_operands      # noqa: F401 (make_operands: for the tests)
from error_bounds import C_DOT, E_TRANS, U32

DEFECTS = ('no_sym', 'apc_missing', 'untrimmed_index', 'wrong_sequence', 'feature_hl', 'col0_ignored', 'scale_d')


def _kept(cu, f, e):
    cu_l, lens = _lens(cu)
    return cu_l, lens, [max(S - f - e, 0) for S in lens]


def make_pairs(lengths, f=1, e=1, seed=0, random_pairs=200):
    """int32 (P, 3) rows (s, i, j): for n <= 18 every (i, j), the diagonal and i > j included; for longer sequences the four corners
    and `random_pairs` seeded random pairs; then ~10 % duplicates, the whole list shuffled."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for s, S in enumerate(lengths):
        n = max(S - f - e, 0)
        if n == 0:
            continue
        if n <= 18:
            ij = torch.cartesian_prod(torch.arange(n), torch.arange(n)).reshape(-1, 2)
        else:
            corners = torch.tensor([[0, 0], [0, n - 1], [n - 1, 0], [n - 1, n - 1]])
            ij = torch.cat((corners, torch.randint(0, n, (random_pairs, 2), generator=g)))
        rows.append(torch.cat((torch.full((ij.shape[0], 1), s), ij), 1))
    pairs = torch.cat(rows)
    dup = pairs[torch.randint(0, pairs.shape[0], (pairs.shape[0] // 10,), generator=g)]
    pairs = torch.cat((pairs, dup))
    return pairs[torch.randperm(pairs.shape[0], generator=g)].to(torch.int32).contiguous()


def _by_sequence(pairs):
    p = pairs.cpu().long()
    return {int(s): (p[:, 0] == s).nonzero().reshape(-1) for s in p[:, 0].unique()}


def reference_features(layers, cu, H, d, scale, pairs, f=1, e=1):
    """float64 (P, L * H) on the operands' device, layer-major columns.  Every pair must be in range."""
    cu_l, lens, ns = _kept(cu, f, e)
    dev = layers[0][0].device
    L = len(layers)
    out = torch.full((pairs.shape[0], L * H), float('nan'), dtype=torch.float64, device=dev)
    pl = pairs.cpu().long()
    for s, idx in _by_sequence(pairs).items():
        a, S, n = cu_l[s], lens[s], ns[s]
        i, j = pl[idx, 1].to(dev), pl[idx, 2].to(dev)
        assert n > 0 and int(i.max()) < n and int(j.max()) < n and int(i.min()) >= 0 and int(j.min()) >= 0
        for l, (q, k, qp) in enumerate(layers):
            sc, _ = _scores2(q, k, qp, a, S, H, d, scale)
            P = torch.softmax(sc * LN2, dim=2)
            A = P[:, f:S - e, f:S - e]
            Y = A + A.transpose(1, 2)
            r = Y.sum(2)
            t = r.sum(1)
            N = Y[:, i, j] - r[:, i] * r[:, j] / t[:, None]                                  # (H, pairs of s)
            out[idx.to(dev), l * H:(l + 1) * H] = N.T
    return out


def feature_bound(layers, cu, H, d, scale, pairs, f=1, e=1):
    """float64 (P, L * H) bound of |kernel - reference_features| for one esme_hip_contact_features call per layer."""
    cu_l, lens, ns = _kept(cu, f, e)
    dev = layers[0][0].device
    L = len(layers)
    out = torch.full((pairs.shape[0], L * H), float('nan'), dtype=torch.float64, device=dev)
    pl = pairs.cpu().long()
    n_dot = 7 + int(math.log2(d // 8))                # [dot]: 7 rounded additions in a lane; [dot-tree]: log2(d / 8) butterfly levels
    for s, idx in _by_sequence(pairs).items():
        a, S, n = cu_l[s], lens[s], ns[s]
        i, j = pl[idx, 1].to(dev), pl[idx, 2].to(dev)
        nk = 4 * ((S + TILE - 1) // TILE) + 4         # additions behind one row sum (contact_bounds.contact_bound)
        nq = 4 * ((n + TILE - 1) // TILE) + 4         # ... behind one column sum
        nt = (n + 63) // 64 + 6                       # [t]
        for l, (q, k, qp) in enumerate(layers):
            sc, nrm = _scores2(q, k, qp, a, S, H, d, scale)
            c = 1.0 if qp else scale * LOG2E
            q64 = q[a:a + S].double().reshape(S, H, d)
            k64 = k[a:a + S].double().reshape(S, H, d)
            l1 = c * torch.einsum('ihc,jhc->hij', q64.abs(), k64.abs())                      # sum_c |q_c k_c| in log2 units
            P = torch.softmax(sc * LN2, dim=2)
            m = sc.max(2, keepdim=True).values
            # --- the statistics passes (MFMA scores, the statistical dot-product form), as in contact_bound
            ds = C_DOT * U32 * math.sqrt(d) * nrm + 3 * U32 * sc.abs()
            eps = LN2 * (ds + U32 * (sc.abs() + m.abs())) + 2 * E_TRANS
            eps_den = (P * eps).sum(2, keepdim=True) + nk * U32                              # [row-sum]
            EA = (P * (eps + eps_den + 2 * U32))[:, f:S - e, f:S - e]
            A = P[:, f:S - e, f:S - e]
            Y = A + A.transpose(1, 2)
            row, col = A.sum(2), A.sum(1)
            r = row + col
            t = r.sum(1)
            d_row = EA.sum(2) + (nk + 2) * U32 * row
            d_col = EA.sum(1) + nq * U32 * col                                               # [col-sum]
            d_r = d_row + d_col + U32 * r                                                    # [r]
            d_t = d_r.sum(1) + nt * U32 * t                                                  # [t]
            # --- the gather pass.  Score: the worst-case FMA-chain form; fp32(scale), fp32(log2 e), their product and [score-scale]
            # are four roundings of |s| (none with a prescaled q, where the factor is exactly 1); [exp]: the fp32 subtraction s - m and
            # exp2f (2 ulp allowed).  The stored maximum cancels between this numerator and the stored denominator.
            ds_g = n_dot * U32 * l1 + (0 if qp else 4) * U32 * sc.abs()
            eps_g = LN2 * (ds_g + U32 * (sc.abs() + m.abs())) + 2 * E_TRANS
            EG = (P * (eps_g + eps_den + 2 * U32))[:, f:S - e, f:S - e]                      # [inv-l] [normalise]: absolute error of one A_ij
            dY = EG[:, i, j] + EG[:, j, i] + U32 * Y[:, i, j]                                # [sym]
            apc = r[:, i] * r[:, j] / t[:, None]
            rel = (d_t / t)[:, None] + (d_r / r)[:, i] + (d_r / r)[:, j] + 2 * U32           # [inv-t], [rr]
            total = dY + apc * rel + U32 * (Y[:, i, j] + apc)                                # [apc]: the one rounding of the fused multiply-add
            out[idx.to(dev), l * H:(l + 1) * H] = (1.01 * total).T                           # 1 %: second-order terms
    return out


# ------------------------------------------------------------------ CPU emulation of the kernel, with defect switches

def emulate_features(layers, cu, H, d, scale, pairs, f=1, e=1, defect=None):
    """float32 emulation of one esme_hip_contact_features call per layer (col0 = l * H) into a zero-filled (P, L * H) matrix.
    `defect`: None or one of DEFECTS."""
    assert defect is None or defect in DEFECTS, defect
    cu_l, lens, ns = _kept(cu, f, e)
    L, B = len(layers), len(lens)
    out = torch.zeros(pairs.shape[0], L * H)
    pl = pairs.cpu().long()
    for s, idx in _by_sequence(pairs).items():
        i, j = pl[idx, 1], pl[idx, 2]
        src = s
        if defect == 'wrong_sequence':                  # rows and statistics of the next sequence that has kept rows
            src = next(x % B for x in range(s + 1, s + 1 + B) if ns[x % B] > 0 and x % B != s)
            i, j = i.clamp(max=ns[src] - 1), j.clamp(max=ns[src] - 1)
        a, S, n = cu_l[src], lens[src], ns[src]
        for l, (q, k, qp) in enumerate(layers):
            sc = 1.0 / d if defect == 'scale_d' else scale
            c = torch.tensor(1.0 if qp and defect != 'scale_d' else sc * LOG2E, dtype=torch.float32)
            if qp and defect == 'scale_d':
                c = torch.tensor(sc / scale, dtype=torch.float32)
            q32 = q[a:a + S].float().cpu().reshape(S, H, d)
            k32 = k[a:a + S].float().cpu().reshape(S, H, d)
            sm = torch.einsum('ihc,jhc->hij', q32, k32) * c
            m = sm.max(2, keepdim=True).values
            p = torch.exp2(sm - m)
            Pn = p * (1.0 / p.sum(2, keepdim=True))
            A = Pn[:, f:S - e, f:S - e]
            r = A.sum(2) + A.sum(1)
            t = r.sum(1)
            ri, rj = (i, j) if defect == 'untrimmed_index' else (i + f, j + f)              # rows of P; untrimmed_index: i, j taken as packed rows
            p1, p2 = Pn[:, ri, rj], Pn[:, rj, ri]
            y = p1 if defect == 'no_sym' else p1 + p2
            v = y if defect == 'apc_missing' else y - (r[:, i] * r[:, j]) * (1.0 / t)[:, None]
            for h in range(H):
                col = h * L + l if defect == 'feature_hl' else (h if defect == 'col0_ignored' else l * H + h)
                out[idx, col] = v[h]
    return out

