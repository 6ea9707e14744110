"""float64 reference, per-element error bound and CPU emulation for the contact kernels (csrc/contacts.hip, include/esme_hip_contacts.h).

`reference_contacts` restates the definition of ESM-2's contact head (Rao et al. 2021) in float64 on the operands the kernel was handed:
per layer l and head h,  P = softmax over ALL S keys of (q_i . k_j) * scale,  A = P[f : S - e, f : S - e],  Y = A + A^T,  r = Y 1,
t = 1^T r,  N = Y - r r^T / t;  logit = b + sum_{l,h} w[l, h] N.  `contact_bound` is the sum of the kernel's rounding steps, each tagged
with the marker of the kernel line that performs it ([score-scale], [exp], ...), with the constants of tests/error_bounds.py.
`emulate_contacts` is a float32 CPU emulation of the kernel's data flow with switches for defects; tests/test_contacts_cpu.py checks that
the bound accepts the correct emulation and rejects each defect.

A layer is a tuple (q, k, q_prescaled): q, k (T, H * d) bf16 (any strides), q_prescaled = q already carries scale * log2(e).
"""
import math

import torch

from error_bounds import C_DOT, E_TRANS, U32

TILE = 64                    # kCT: tile edge (contacts.hip)
LOG2E = 1.0 / math.log(2.0)
LN2 = math.log(2.0)

DEFECTS = ('apc_untrimmed', 'softmax_trimmed', 'no_sym', 'r_rows_only', 'feature_hl', 'scale_d', 'col_next_seq', 'col_tail_missing', 'p_bf16')


def _lens(cu):
    cu = [int(c) for c in cu.cpu()]
    return cu, [b - a for a, b in zip(cu[:-1], cu[1:])]


def _scores2(q, k, qp, a, S, H, d, scale):
    """float64 scores in log2 units (H, S, S) of rows a .. a + S - 1, and sqrt(sum_c (q_c k_c)^2) for the dot-product term."""
    q64 = q[a:a + S].double().reshape(S, H, d)
    k64 = k[a:a + S].double().reshape(S, H, d)
    c = 1.0 if qp else scale * LOG2E
    s = c * torch.einsum('ihc,jhc->hij', q64, k64)
    nrm = c * torch.sqrt(torch.einsum('ihc,jhc->hij', q64 * q64, k64 * k64))
    return s, nrm


def reference_contacts(layers, cu, H, d, scale, w, bias, f=1, e=1):
    """List of B float64 (n_s, n_s) logit maps; w (L, H) in layer-major feature order."""
    cu_l, lens = _lens(cu)
    w64 = w.double().reshape(len(layers), H)
    out = []
    for a, S in zip(cu_l, lens):
        n = max(S - f - e, 0)
        dev = layers[0][0].device
        logit = torch.full((n, n), float(bias), dtype=torch.float64, device=dev)
        if n:
            for l, (q, k, qp) in enumerate(layers):
                s, _ = _scores2(q, k, qp, a, S, H, d, scale)
                P = torch.softmax(s * LN2, dim=2)                           # softmax of the natural-unit scores over all S keys
                A = P[:, f:S - e, f:S - e]
                Y = A + A.transpose(1, 2)
                r = Y.sum(2)
                t = r.sum(1)
                N = Y - r[:, :, None] * r[:, None, :] / t[:, None, None]
                logit = logit + torch.einsum('h,hij->ij', w64[l].to(dev), N)
        out.append(logit)
    return out


def contact_bound(layers, cu, H, d, scale, w, bias, f=1, e=1):
    """List of B float64 (n_s, n_s) bounds of |kernel - reference_contacts| for one esme_hip_contact_layer call per layer."""
    cu_l, lens = _lens(cu)
    L = len(layers)
    w64 = w.double().reshape(L, H)
    out = []
    for a, S in zip(cu_l, lens):
        n = max(S - f - e, 0)
        dev = layers[0][0].device
        total = torch.zeros((n, n), dtype=torch.float64, device=dev)
        mag = torch.full((n, n), abs(float(bias)), dtype=torch.float64, device=dev)
        if n:
            nk = 4 * ((S + TILE - 1) // TILE) + 4       # additions behind one row sum: 4 per key tile in a lane, then the 16-lane butterfly
            nq = 4 * ((n + TILE - 1) // TILE) + 4       # the same for a column sum over the kept query tiles
            nt = (n + 63) // 64 + 6                     # [t]: rows per lane, then the 64-lane butterfly
            for l, (q, k, qp) in enumerate(layers):
                s, nrm = _scores2(q, k, qp, a, S, H, d, scale)
                wl = w64[l].to(dev).abs()[:, None, None]
                P = torch.softmax(s * LN2, dim=2)
                m = s.max(2, keepdim=True).values
                # score in log2 units: the MFMA's fp32 accumulation of d exact products (statistical form), fp32(scale) * fp32(log2 e) and
                # [score-scale] (three roundings of |s|); [exp]: the fp32 subtraction s - m and exp2f (2 ulp allowed).  The stored maximum
                # itself cancels between numerator and denominator, which all three passes form with the same m.
                ds = C_DOT * U32 * math.sqrt(d) * nrm + 3 * U32 * s.abs()
                eps = LN2 * (ds + U32 * (s.abs() + m.abs())) + 2 * E_TRANS                  # relative error of one exp2(s - m)
                # [row-sum]: nk additions of positive terms; [inv-l] one division; [normalise] one multiplication
                eps_den = (P * eps).sum(2, keepdim=True) + nk * U32
                EA = (P * (eps + eps_den + 2 * U32))[:, f:S - e, f:S - e]                   # absolute error of one A_ij
                A = P[:, f:S - e, f:S - e]
                Y = A + A.transpose(1, 2)
                row, col = A.sum(2), A.sum(1)
                r = row + col
                t = r.sum(1)
                dY = EA + EA.transpose(1, 2) + U32 * Y                                       # [sym]
                d_row = EA.sum(2) + (nk + 2) * U32 * row                                     # the kept keys' sum, [inv-l], [normalise]
                d_col = EA.sum(1) + nq * U32 * col                                           # [col-sum]
                d_r = d_row + d_col + U32 * r                                                # [r]
                d_t = d_r.sum(1) + nt * U32 * t                                              # [t]
                apc = r[:, :, None] * r[:, None, :] / t[:, None, None]
                rel = (d_t / t)[:, None, None] + (d_r / r)[:, :, None] + (d_r / r)[:, None, :] + 3 * U32      # [w-over-t], r_i * r_j, [apc]
                M = (wl * (Y + apc)).sum(0)                                                  # what the head sum's partial sums can reach
                total = total + (wl * (dY + apc * rel)).sum(0) + 2 * H * U32 * M             # [head-sum]: 2 H fused multiply-adds
                mag = mag + M
            total = 1.01 * total + L * U32 * mag                                             # 1 %: second-order terms; [layer-sum]
        out.append(total)
    return out


# ------------------------------------------------------------------ CPU emulation of the kernel, with defect switches

def emulate_contacts(layers, cu, H, d, scale, w, bias, f=1, e=1, defect=None):
    """float32 emulation of one esme_hip_contact_layer call per layer; returns B float32 (n_s, n_s) maps.  `defect`: None or one of DEFECTS."""
    assert defect is None or defect in DEFECTS, defect
    cu_l, lens = _lens(cu)
    L = len(layers)
    w32 = w.float().reshape(L, H).cpu()
    T = layers[0][0].shape[0]
    out = []
    for a, S in zip(cu_l, lens):
        n = max(S - f - e, 0)
        if n == 0:
            out.append(torch.zeros(0, 0))
            continue
        acc_map = None
        for l, (q, k, qp) in enumerate(layers):
            sc = 1.0 / d if defect == 'scale_d' else scale
            c = torch.tensor(1.0 if qp and defect != 'scale_d' else sc * LOG2E, dtype=torch.float32)
            if qp and defect == 'scale_d':
                c = torch.tensor(sc / scale, dtype=torch.float32)
            extra = min(2, T - (a + S)) if defect == 'col_next_seq' else 0
            q32 = q[a:a + S + extra].float().cpu().reshape(S + extra, H, d)
            k32 = k[a:a + S].float().cpu().reshape(S, H, d)
            s = torch.einsum('ihc,jhc->hij', q32, k32) * c                                  # (H, S + extra, S)
            if defect == 'softmax_trimmed':
                s = s[:, :, f:S - e]
                lo, hi = 0, n
            else:
                lo, hi = f, S - e
            m = s.max(2, keepdim=True).values
            p = torch.exp2(s - m)
            inv = 1.0 / p.sum(2, keepdim=True)
            Pn = p * inv
            if defect == 'p_bf16':
                Pn = Pn.to(torch.bfloat16).float()
            acc = torch.zeros(n, n)
            for h in range(H):
                wh = w32.reshape(-1)[h * L + l] if defect == 'feature_hl' else w32[l, h]
                if defect == 'apc_untrimmed':
                    Yf = Pn[h, :S] + Pn[h, :S].T
                    rf = Yf.sum(1)
                    Nf = Yf - rf[:, None] * rf[None, :] / rf.sum()
                    acc = acc + wh * Nf[f:S - e, f:S - e]
                    continue
                A = Pn[h, f:S - e, lo:hi]
                row = A.sum(1)
                colsrc = Pn[h, f:S - e + extra, lo:hi] if extra else A
                col = colsrc.sum(0)
                if defect == 'col_tail_missing' and n % TILE:
                    col = col.clone()
                    col[n // TILE * TILE:] = 0.0
                Y = A if defect == 'no_sym' else A + A.T
                r = row if defect == 'r_rows_only' else (Y.sum(1) if defect == 'no_sym' else row + col)
                t = r.sum()
                acc = acc + wh * Y
                acc = acc - (wh / t) * (r[:, None] * r[None, :])
            acc_map = (torch.tensor(float(bias)) + acc) if acc_map is None else acc_map + acc
        out.append(acc_map)
    return out


def make_operands(lengths, H, d, seed, score_std=1.5, logical_d=None, qp=False, layers=2, device='cpu'):
    """q, k column views of one (T, 3 H d) bf16 buffer per layer with natural-unit scores of standard deviation ~score_std; pad lanes
    (logical_d .. d - 1 of every head) zero.  Returns (layers, cu_lens int32, scale)."""
    g = torch.Generator().manual_seed(seed)
    T, E = sum(lengths), H * d
    ld = logical_d or d
    scale = ld ** -0.5
    cu = torch.zeros(len(lengths) + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(torch.tensor(lengths), 0)
    out = []
    for _ in range(layers):
        qkv = torch.randn(T, 3, H, d, generator=g) * math.sqrt(score_std)
        qkv[..., ld:] = 0.0
        if qp:
            qkv[:, 0] *= scale * LOG2E
        qkv = qkv.to(torch.bfloat16).reshape(T, 3 * E).to(device)
        out.append((qkv[:, :E], qkv[:, E:2 * E], qp))
    return out, cu.to(device), scale
