"""float64 reference, per-element error bound and CPU emulation for esme_hip_attn_maps (csrc/attn_maps.hip, include/esme_hip_attn_maps.h).

`reference_maps` restates the definition in float64 on the bf16 operands the kernel was handed: per layer l and listed head h,
P = softmax over ALL S keys of (q_i . k_j) * scale, bos / eos rows and columns included; with head weights sum_j w[l, j] P^(heads[j]).
`map_bound` is the sum of the kernel's rounding steps, each tagged with the marker of the kernel line that performs it ([score-scale],
[exp], ...), with the constants of tests/error_bounds.py; there is no rms floor.  `emulate_maps` is a float32 CPU emulation of the
kernel's order of operations with switches for defects; tests/test_attn_maps_cpu.py checks that the bound accepts the correct emulation
and rejects each defect wherever it applies (`defect_applies`).

A layer is a tuple (q, k, q_prescaled): q, k (T, H * d) bf16 (any strides), q_prescaled = q already carries scale * log2(e).
Results are lists of B tensors, one per sequence: (L, n, S, S) for the n listed heads, (L, S, S) with head weights -- the block layout
model.attention_maps returns (the i-th selected layer's call writes slots i * n_out ..).
"""
import math

import torch

from contact_bounds import LN2, LOG2E, TILE, _lens, _scores2
from error_bounds import E_TRANS, C_DOT, U32

TINY = 2.0 ** -126           # exp2 of a result below the smallest normal fp32 may be flushed to zero

DEFECTS = ('no_scale', 'next_seq_keys', 'transposed', 'head_plus_1', 'unnormalised', 'tile_local_max', 'tail_dropped', 'head_minor_slots',
           'weights_ignored', 'bf16_truncated')


def defect_applies(defect, S, T_after, H, L, n, weighted, out_bf16, qp):
    """Can `defect` change the maps of a sequence of S rows (T_after packed rows follow it; H heads, L layers, n listed heads)?
     - no_scale           not with a prescaled q (the kernel then applies no scale of its own), not at S = 1 (P = 1 whatever the scores);
     - next_seq_keys      only where rows follow the sequence in the packed buffer;
     - transposed, head_plus_1, unnormalised, bf16_truncated: not at S = 1 (the one entry is 1); head_plus_1 needs H > 1;
     - tile_local_max     only with more than one key tile (S > 64);
     - tail_dropped       only with a partial last key tile (S % 64 != 0);
     - head_minor_slots   only with several layers and several blocks per layer, not at S = 1;
     - weights_ignored    only in weighted mode;  bf16_truncated only with bf16 output."""
    if S == 0:
        return False
    return {'no_scale': not qp and S > 1, 'next_seq_keys': T_after > 0, 'transposed': S > 1, 'head_plus_1': S > 1 and H > 1,
            'unnormalised': S > 1, 'tile_local_max': S > TILE, 'tail_dropped': S % TILE != 0,
            'head_minor_slots': L > 1 and n > 1 and not weighted and S > 1, 'weights_ignored': weighted,
            'bf16_truncated': out_bf16 and S > 1}[defect]


def _half_ulp_bf16(x):
    """Half a bf16 ulp at magnitude x (float64, > 0): x = m 2^e with m in [0.5, 1) has ulp 2^(e - 8)."""
    _, e = torch.frexp(x)
    return torch.ldexp(torch.ones_like(x), e - 9)


def reference_maps(layers, cu, H, d, scale, heads, weights=None):
    cu_l, lens = _lens(cu)
    out = []
    for a, S in zip(cu_l, lens):
        per_layer = []
        for l, (q, k, qp) in enumerate(layers):
            s, _ = _scores2(q, k, qp, a, S, H, d, scale)
            P = torch.softmax(s * LN2, dim=2)[heads] if S else s[heads]      # softmax of the natural-unit scores over all S keys
            if weights is not None:
                P = torch.einsum('j,jik->ik', weights[l].double().to(P.device), P)
            per_layer.append(P)
        out.append(torch.stack(per_layer))
    return out


def map_bound(layers, cu, H, d, scale, heads, weights=None, out_bf16=False):
    """List of B float64 bounds of |kernel - reference_maps|, in the shapes of reference_maps."""
    cu_l, lens = _lens(cu)
    n = len(heads)
    out = []
    for a, S in zip(cu_l, lens):
        nk = 4 * ((S + TILE - 1) // TILE) + 4           # additions behind one row sum: 4 per key tile in a lane, then the 16-lane butterfly
        per_layer = []
        for l, (q, k, qp) in enumerate(layers):
            s, nrm = _scores2(q, k, qp, a, S, H, d, scale)
            if not S:
                per_layer.append(s[heads] if weights is None else s[0])
                continue
            s, nrm = s[heads], nrm[heads]
            P = torch.softmax(s * LN2, dim=2)
            m = s.max(2, keepdim=True).values
            # score in log2 units: the MFMA's fp32 accumulation of d exact products (statistical form), fp32(scale) * fp32(log2 e) and
            # [score-scale] (three roundings of |s|); [exp]: the fp32 subtraction s - m and exp2f (2 ulp allowed).  The stored maximum
            # itself cancels between numerator and denominator: both kernels form exp2(s - m) with the same m.
            ds = C_DOT * U32 * math.sqrt(d) * nrm + 3 * U32 * s.abs()
            eps = LN2 * (ds + U32 * (s.abs() + m.abs())) + 2 * E_TRANS                      # relative error of one exp2(s - m)
            # [row-sum]: nk additions of positive terms; [inv-l] one division; [normalise] one multiplication
            eps_den = (P * eps).sum(2, keepdim=True) + nk * U32
            EP = 1.01 * P * (eps + eps_den + 2 * U32) + TINY                                # 1 %: second-order terms
            if weights is None:
                ref, E = P, EP
            else:
                w = weights[l].double().to(P.device)[:, None, None]
                ref = (w * P).sum(0).abs()
                mag = (w.abs() * P).sum(0)                                                   # what the head sum's partial sums can reach
                E = (w.abs() * EP).sum(0) + n * U32 * mag                                    # [head-sum]: n fused multiply-adds
            if out_bf16:
                E = E + _half_ulp_bf16(ref + E)                                              # [out-round]: half an ulp of the fp32 value
            per_layer.append(E)
        out.append(torch.stack(per_layer))
    return out


# ------------------------------------------------------------------ CPU emulation of the kernel, with defect switches

def _truncate_bf16(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def emulate_maps(layers, cu, H, d, scale, heads, weights=None, out_bf16=False, defect=None):
    """float32 emulation of one esme_hip_attn_maps call per layer (slot0 = l * n_out); returns B float32 tensors in the shapes of
    reference_maps (bf16 output: the bf16 values, widened).  `defect`: None or one of DEFECTS."""
    assert defect is None or defect in DEFECTS, defect
    cu_l, lens = _lens(cu)
    L, n = len(layers), len(heads)
    T = layers[0][0].shape[0]
    out = []
    for a, S in zip(cu_l, lens):
        n_out = 1 if weights is not None else n
        if S == 0:
            out.append(torch.zeros((L, 0, 0) if weights is not None else (L, n, 0, 0)))
            continue
        slots = torch.zeros(L * n_out, S, S)
        for l, (q, k, qp) in enumerate(layers):
            c = torch.tensor(1.0 if qp else (LOG2E if defect == 'no_scale' else scale * LOG2E), dtype=torch.float32)
            extra = min(2, T - (a + S)) if defect == 'next_seq_keys' else 0
            q32 = q[a:a + S].float().cpu().reshape(S, H, d)
            k32 = k[a:a + S + extra].float().cpu().reshape(S + extra, H, d)
            hs = [(h + 1) % H for h in heads] if defect == 'head_plus_1' else list(heads)
            s = torch.einsum('ihc,jhc->hij', q32[:, hs], k32[:, hs]) * c                   # (n, S, S + extra)      [score-scale]
            keep = S + extra
            if defect == 'tail_dropped':
                keep = S // TILE * TILE
            if defect == 'tile_local_max':
                m = torch.cat([s[:, :, t:t + TILE].max(2, keepdim=True).values.expand(-1, -1, min(TILE, S - t)) for t in range(0, S, TILE)], 2)
            else:
                m = s[:, :, :max(keep, 1)].max(2, keepdim=True).values
            p = torch.exp2(s - m)                                                           # [exp]
            p[:, :, keep:] = 0.0
            lsum = p.sum(2, keepdim=True)                                                   # [row-sum]
            inv = torch.where(lsum > 0, 1.0 / lsum, torch.zeros_like(lsum))                # [inv-l]
            P = (p if defect == 'unnormalised' else p * inv)[:, :, :S]                      # [normalise]
            if defect == 'transposed':
                P = P.transpose(1, 2)
            if weights is not None:
                acc = torch.zeros(S, S)
                for j in range(n):                                                          # [head-sum], in list order
                    acc = acc + weights[l, j].float().cpu() * P[j]
                if defect == 'weights_ignored':
                    acc = P[0]
                P = acc[None]
            for j in range(n_out):
                slot = j * L + l if defect == 'head_minor_slots' else l * n_out + j
                slots[slot] = P[j]
        if out_bf16:                                                                        # [out-round]
            slots = _truncate_bf16(slots) if defect == 'bf16_truncated' else slots.to(torch.bfloat16).float()
        out.append(slots.view((L, S, S) if weights is not None else (L, n, S, S)))
    return out


def make_operands(lengths, H, d, seed, logical_d=None, qp=False, score_std=3.0, layers=1, device='cpu'):
    """q, k column views of one (T, 3 H d) bf16 buffer per layer with natural-unit scores of standard deviation ~score_std (peaked rows:
    the largest entry of every sequence stands far above every bound); pad lanes (logical_d .. d - 1 of every head) zero.
    Returns (layers, cu_lens int32, scale)."""
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


def worst_ratio(got, ref, bound):
    """Per sequence: max |got - ref| / bound (0.0 for an empty sequence)."""
    return [float(((g.double() - r).abs() / b).max()) if r.numel() else 0.0 for g, r, b in zip(got, ref, bound)]


def signal_over_bound(ref, bound):
    """(the smallest, over the non-empty sequences, of the largest |map entry|) / (the largest bound of the batch)."""
    top = max(float(b.max()) for b in bound if b.numel())
    return min(float(r.abs().max()) for r in ref if r.numel()) / top
