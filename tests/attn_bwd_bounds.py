"""float64 reference, per-element error bound and CPU emulation for the attention backward (csrc/attn_bwd.hip, include/esme_hip_attn_bwd.h),
in the manner of contact_bounds.py / lora_bounds.py.

`reference_bwd` states the gradients of O = softmax(Q K^T scale) V in float64 on the bf16 operands the kernel is handed (q, k, v, dO):
        P = softmax_j(scale q_i . k_j),  dP = dO V^T,  D_i = sum_c dO_ic O_ic (O = P V in float64),  dS = P o (dP - D),
        dV = P^T dO,  dQ = scale dS K,  dK = scale dS^T Q.
`bwd_bound` is the sum of the kernel's rounding steps, per element, with the constants of tests/error_bounds.py:
  [score]   S in log2 units: the MFMA's fp32 accumulation of d exact products (eb.dot_term's statistical form), fp32(scale) * fp32(log2 e)
            and the product with it (three roundings of |s|);
  [exp]     the score error carried through exp2: ln 2 * (score error + the fp32 subtraction s - m) + exp2f (2 ulp allowed); the row sum's
            additions, one division, one product -- the relative error of P, as contact_bounds.py prices it;
  [dP]      eb.dot_term of dO . v over d;
  [D]       D is taken from the bf16 `o` that is handed in, not from the exact O: sum_c |dO_ic| |o_ic - O_ic|, plus its own fp32
            accumulation (d / 4 fused multiply-adds per lane and two additions);
  [dS]      the fp32 subtraction dP - D and the product with P;
  [bf16]    P and dS rounded to bf16 where they become MFMA operands: 2^-8 relative each;
  [acc]     eb.dot_term of the three products over the sequence (P^T dO, dS K, dS^T Q), and the product with softmax_scale;
  [out]     the rounding of every output to bf16, once.
`emulate_bwd` restates the kernel path in fp32 / bf16 on the CPU and can inject the defects a review would look for (DEFECTS);
tests/test_attn_bwd_cpu.py checks that the bound accepts the faithful emulation and rejects each of them on the GPU test's shapes.
"""
import math

import torch

import error_bounds as eb
from error_bounds import C_DOT, E_TRANS, U32

TILE = 64
LOG2E = 1.0 / math.log(2.0)
LN2 = math.log(2.0)
U_BF = 2.0 ** -8        # bf16 unit roundoff: half an ulp (2^-8 of the binade's lower edge) relative to the value

LENGTHS = (0, 1, 2, 63, 64, 65, 129, 0, 200)        # the GPU test's batch: the tile edges and empty sequences
HEADS = 3

DEFECTS = ('no_scale', 'no_D', 'D_next_head', 'key_next_seq', 'p_unnormalised', 'ds_untransposed')


def _lens(cu):
    cu = [int(c) for c in cu.cpu()]
    return cu, [b - a for a, b in zip(cu[:-1], cu[1:])]


def _heads(t, a, S, H, d):
    """rows a .. a + S - 1 of a (T, H * d) tensor as float64 (H, S, d)"""
    return t[a:a + S].double().reshape(S, H, d).transpose(0, 1)


def _flat(x):
    """(H, S, d) -> (S, H * d)"""
    return x.transpose(0, 1).reshape(x.shape[1], -1)


def _seq64(q, k, v, do, a, S, H, d, scale):
    Q, K, V, G = (_heads(t, a, S, H, d) for t in (q, k, v, do))
    s2 = scale * LOG2E * (Q @ K.transpose(1, 2))                     # log2 units
    P = torch.softmax(s2 * LN2, dim=2)
    O = P @ V
    dP = G @ V.transpose(1, 2)
    D = (G * O).sum(2, keepdim=True)
    dS = P * (dP - D)
    return Q, K, V, G, s2, P, O, dP, D, dS


def reference_bwd(q, k, v, do, cu, H, d, scale):
    """(dq, dk, dv, o) float64 (T, H * d)."""
    cu_l, lens = _lens(cu)
    out = [torch.zeros(q.shape, dtype=torch.float64) for _ in range(4)]
    for a, S in zip(cu_l, lens):
        if S == 0:
            continue
        Q, K, V, G, s2, P, O, dP, D, dS = _seq64(q, k, v, do, a, S, H, d, scale)
        for dst, val in zip(out, (scale * (dS @ K), scale * (dS.transpose(1, 2) @ Q), P.transpose(1, 2) @ G, O)):
            dst[a:a + S] = _flat(val)
    return tuple(out)


def _acc(x, y, n):
    """[acc]: fp32 accumulation of sum_n x[., n] y[n, .] (statistical form of eb.dot_term); x (H, R, n), y (H, n, C)"""
    return C_DOT * U32 * math.sqrt(n) * torch.sqrt(torch.clamp((x * x) @ (y * y), min=0.0))


def bwd_bound(q, k, v, o, do, cu, H, d, scale):
    """(bound of dq, of dk, of dv) float64 (T, H * d) for |kernel - reference_bwd|; `o` is the bf16 output the kernel is handed."""
    cu_l, lens = _lens(cu)
    out = [torch.zeros(q.shape, dtype=torch.float64) for _ in range(3)]
    for a, S in zip(cu_l, lens):
        if S == 0:
            continue
        Q, K, V, G, s2, P, O, dP, D, dS = _seq64(q, k, v, do, a, S, H, d, scale)
        ob = _heads(o, a, S, H, d)
        nk = 4 * ((S + TILE - 1) // TILE) + 4                        # additions behind one row sum (contact_bounds.py)
        nrm = scale * LOG2E * torch.sqrt((Q * Q) @ (K * K).transpose(1, 2))
        m = s2.max(2, keepdim=True).values
        e_s = C_DOT * U32 * math.sqrt(d) * nrm + 3 * U32 * s2.abs()                                  # [score]
        eps = LN2 * (e_s + U32 * (s2.abs() + m.abs())) + 2 * E_TRANS                                 # [exp]
        eps_den = (P * eps).sum(2, keepdim=True) + nk * U32
        EP = P * (eps + eps_den + 2 * U32)
        EPb = EP + U_BF * (P + EP)                                                                   # [bf16] P
        EdP = C_DOT * U32 * math.sqrt(d) * torch.sqrt((G * G) @ (V * V).transpose(1, 2))             # [dP]
        ED = (G.abs() * (ob - O).abs()).sum(2, keepdim=True) + (d // 4 + 2) * U32 * (G * ob).abs().sum(2, keepdim=True)      # [D]
        EdS = EP * (dP - D).abs() + (P + EP) * (EdP + ED + U32 * (dP - D).abs()) + U32 * dS.abs()    # [dS]
        EdSb = EdS + U_BF * (dS.abs() + EdS)                                                         # [bf16] dS
        Pt, dSt = P.transpose(1, 2), dS.transpose(1, 2)
        vals = (scale * (dS @ K), scale * (dSt @ Q), Pt @ G)
        pres = (scale * (EdSb @ K.abs() + _acc(dS, K, S)) + U32 * vals[0].abs(),                     # [acc]
                scale * (EdSb.transpose(1, 2) @ Q.abs() + _acc(dSt, Q, S)) + U32 * vals[1].abs(),
                EPb.transpose(1, 2) @ G.abs() + _acc(Pt, G, S))
        for dst, val, pre in zip(out, vals, pres):
            pre = 1.01 * pre                                                                         # 1 %: second-order terms
            dst[a:a + S] = _flat(pre + eb.out_round(val, pre, 'bf16'))                               # [out]
    return tuple(out)


# ------------------------------------------------------------------ CPU emulation of the kernel, with defect switches

def _mm32(x, y):
    """fp32 result of an exact-product matrix product (float64 accumulation stands in for the MFMA's fp32 chain)"""
    return (x.double() @ y.double()).float()


def _bf(t):
    return t.to(torch.bfloat16).float()


def emulate_bwd(q, k, v, o, do, cu, H, d, scale, defect=None):
    """fp32 / bf16 emulation of esme_hip_attn_varlen_bwd; returns bf16 (dq, dk, dv) (T, H * d).  `defect`: None or one of DEFECTS."""
    assert defect is None or defect in DEFECTS, defect
    cu_l, lens = _lens(cu)
    T = q.shape[0]
    out = [torch.zeros(q.shape, dtype=torch.bfloat16) for _ in range(3)]
    cs = torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    out_scale = 1.0 if defect == 'no_scale' else torch.tensor(scale, dtype=torch.float32)
    for a, S in zip(cu_l, lens):
        if S == 0:
            continue
        extra = min(1, T - (a + S)) if defect == 'key_next_seq' else 0                     # a key row of the next sequence in the last tile
        Q, G, Ob = (_heads(t, a, S, H, d).float() for t in (q, do, o))
        K, V = (_heads(t, a, S + extra, H, d).float() for t in (k, v))
        s = _mm32(Q, K.transpose(1, 2)) * cs
        m = s.max(2, keepdim=True).values
        p = torch.exp2(s - m)
        P = p if defect == 'p_unnormalised' else p * (1.0 / p.sum(2, keepdim=True))
        dP = _mm32(G, V.transpose(1, 2))
        D = (G * Ob).sum(2, keepdim=True)
        if defect == 'no_D':
            D = torch.zeros_like(D)
        elif defect == 'D_next_head':
            D = torch.roll(D, -1, 0)
        dS = P * (dP - D)
        Pb, dSb = _bf(P), _bf(dS)
        dV = _mm32(Pb.transpose(1, 2), G)[:, :S]
        dQ = _mm32(dSb, K) * out_scale
        dK = (_mm32(dSb if defect == 'ds_untransposed' else dSb.transpose(1, 2), Q) * out_scale)[:, :S]
        for dst, val in zip(out, (dQ, dK, dV)):
            dst[a:a + S] = _flat(val).to(torch.bfloat16)
    return tuple(out)


def forward_bf16(q, k, v, cu, H, d, scale):
    """The bf16 rounding of the float64 attention output: what stands in for the forward kernel's `o` without a device."""
    return reference_bwd(q, k, v, torch.zeros_like(q), cu, H, d, scale)[3].to(torch.bfloat16)


def make_operands(lengths, H, d, seed, score_std=1.5, qk_gain=1.0, device='cpu'):
    """q, k, v column views of one (T, 3 H d) bf16 buffer with natural-unit scores of standard deviation ~score_std (times qk_gain^2), a
    bf16 dO with its own row stride, cu_lens int32 and the softmax scale."""
    g = torch.Generator().manual_seed(seed)
    T, E = sum(lengths), H * d
    scale = d ** -0.5
    cu = torch.zeros(len(lengths) + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(torch.tensor(lengths), 0)
    qkv = torch.randn(T, 3, H, d, generator=g) * math.sqrt(score_std)
    qkv[:, :2] *= qk_gain
    qkv = qkv.to(torch.bfloat16).reshape(T, 3 * E).to(device)
    do = torch.randn(T, E + 8, generator=g).to(torch.bfloat16).to(device)[:, :E]
    return {'q': qkv[:, :E], 'k': qkv[:, E:2 * E], 'v': qkv[:, 2 * E:], 'qkv': qkv, 'do': do, 'cu': cu.to(device), 'scale': scale, 'H': H, 'd': d,
            'lengths': tuple(lengths)}


def worst(got, ref, bound):
    """max over the three gradients of err / bound"""
    return max(float(((g.double().cpu() - r).abs() / b.clamp_min(1e-300)).max()) if r.numel() else 0.0 for g, r, b in zip(got, ref, bound))
