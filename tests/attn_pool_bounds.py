"""float64 references and per-element error bounds for the attention-pooling kernels (csrc/pool.hip) and the heads built on them.

`reference_pool` restates the reference's definition (esme/pooling.py:81-136): k = embed W_k^T + b_k over every row, one query per
(class token, head), softmax(q k^T / sqrt(d)) v with v = embed, in float64 on the operands the kernel was handed.  `pool_bound` is the
sum of the kernel's rounding steps, each tagged with the marker of the kernel line that performs it ([fold-scale], [score], ...), in the
style of tests/error_bounds.py (whose constants and helpers it uses).  `emulate_pool` is a float32 CPU emulation of the kernel with
switches for defects; tests/test_attn_pool_cpu.py checks that the bound accepts the correct emulation and rejects each defect.
"""
import math

import torch

from error_bounds import C_DOT, E_TRANS, U32, dot_term, gemm_reference, out_round

ROWS = 64                   # kPoolRows: rows per chunk (pool.hip)
LOG2E = 1.0 / math.log(2.0)


def _segments(cu):
    cu = cu.to(torch.long).cpu()
    lens = cu[1:] - cu[:-1]
    return cu, lens


def reference_pool(x, cu, cls, wk, bk, heads):
    """(B, C, E) float64: the reference's data flow, literally -- k projected with its bias, per (c, h) softmax over each sequence's
    rows of q . k / sqrt(d), weights applied to the raw embed.  Also returns the per-row probabilities p (T, C, H) for the bound."""
    x64, W, b, q = x.double(), wk.double(), bk.double(), cls.double()
    T, E = x64.shape
    C, H = q.shape[0], heads
    d = E // H
    cu_l, lens = _segments(cu)
    B = lens.numel()
    dev = x64.device
    seg = torch.repeat_interleave(torch.arange(B, device=dev), lens.to(dev))
    k = (x64 @ W.T + b).view(T, H, d)                                    # esme/pooling.py:114  k = self.k(embed)
    scores = torch.einsum('thd,chd->tch', k, q.view(C, H, d)) / math.sqrt(d)
    mx = torch.full((B, C, H), -math.inf, dtype=torch.float64, device=dev)
    mx = mx.scatter_reduce(0, seg.view(-1, 1, 1).expand(T, C, H), scores, 'amax')
    e = torch.exp(scores - mx[seg])
    den = torch.zeros(B, C, H, dtype=torch.float64, device=dev).index_add_(0, seg, e)
    p = e / den[seg]
    v = x64.view(T, H, d)
    out = torch.zeros(B, C, H, d, dtype=torch.float64, device=dev)
    for c in range(C):
        out[:, c] = torch.zeros(B, H, d, dtype=torch.float64, device=dev).index_add_(0, seg, p[:, c, :, None] * v)
    return out.view(B, C, E), p


def folded_scores(x, cls, wk, heads):
    """float64 u_{c,h} . x_t / sqrt(d) (the kernel's algebra, no bias): (T, C, H)."""
    x64, W, q = x.double(), wk.double(), cls.double()
    E = x64.shape[1]
    C, H, d = q.shape[0], heads, E // heads
    u = torch.einsum('chd,hde->che', q.view(C, H, d), W.view(H, d, E))
    return torch.einsum('te,che->tch', x64, u) / math.sqrt(d)


def pool_bound(x, cu, cls, wk, heads, ref, p, out_fmt):
    """Per-element bound (B, C, E) of |got - ref| for esme_hip_attn_pool after esme_hip_attn_pool_fold on these operands."""
    x64, W, q = x.double(), wk.double(), cls.double()
    T, E = x64.shape
    C, H = q.shape[0], heads
    d = E // H
    dev = x64.device
    cu_l, lens = _segments(cu)
    B = lens.numel()
    seg = torch.repeat_interleave(torch.arange(B, device=dev), lens.to(dev))
    scale = LOG2E / math.sqrt(d)
    qh, Wh = q.view(C, H, d), W.view(H, d, E)
    U = scale * torch.einsum('chd,hde->che', qh, Wh)                     # log2 units
    # [fold-scale] fp32 fmaf chain over d products, then fp32(scale) (one rounding) times it (one rounding)
    dU = (scale * C_DOT * U32 * math.sqrt(d) * torch.sqrt(torch.einsum('chd,hde->che', qh * qh, Wh * Wh))
          + 2 * U32 * U.abs())
    s = torch.einsum('te,che->tch', x64, U)
    # [score] fp32 fmaf chain over E exact products U_e x_e, on the fold's U
    ds = (torch.einsum('te,che->tch', x64.abs(), dU)
          + C_DOT * U32 * math.sqrt(E) * torch.sqrt(torch.einsum('te,che->tch', x64 * x64, U * U)))
    idx = seg.view(-1, 1, 1).expand(T, C, H)
    ds_max = torch.zeros(B, C, H, dtype=torch.float64, device=dev).scatter_reduce(0, idx, ds, 'amax')
    s_max = torch.zeros(B, C, H, dtype=torch.float64, device=dev).scatter_reduce(0, idx, s.abs(), 'amax')
    # relative error of each unnormalised weight: its score error and the max row's (the max cancels only when exact); the fp32
    # subtraction s - m [exp] and m_k - M [combine-exp] (|.| <= |s| + 3 max|s|); one v_exp_f32 in each of [exp] and [combine-exp]
    eps = (math.log(2.0) * (ds + ds_max[seg] + U32 * (s.abs() + 3 * s_max[seg])) + 2 * E_TRANS)
    v = x64.view(T, H, d)
    refv = ref.double().view(B, C, H, d)
    nr = torch.clamp(lens, max=ROWS).to(dev).double()
    nch = torch.div(lens + ROWS - 1, ROWS, rounding_mode='floor').to(dev).double()
    n_acc = (nr + nch).view(B, 1, 1, 1)
    pre = torch.zeros(B, C, H, d, dtype=torch.float64, device=dev)
    for c in range(C):
        pc = p[:, c]                                                     # (T, H)
        t1 = torch.zeros(B, H, d, dtype=torch.float64, device=dev).index_add_(
            0, seg, (pc * eps[:, c])[:, :, None] * (v - refv[seg, c]).abs())
        spx = torch.zeros(B, H, d, dtype=torch.float64, device=dev).index_add_(0, seg, pc[:, :, None] * v.abs())
        # [pv] / [row-sum]: fmaf chains of <= 64 positive terms per chunk; [combine-sum]: one fmaf per chunk; numerator and
        # denominator alike.  [divide]: one rounding.
        t2 = U32 * n_acc[:, 0] * (spx + refv[:, c].abs()) + U32 * refv[:, c].abs()
        pre[:, c] = t1 + t2
    pre = 1.01 * pre.view(B, C, E)          # 1 %: the second-order terms of the first-order sum above (eps < 1e-3)
    empty = (lens == 0).to(dev).view(B, 1, 1)
    pre = torch.where(empty, torch.zeros_like(pre), pre)
    # [out-round] one rounding to the output dtype
    return pre + out_round(ref, pre, out_fmt), pre


def check_pool_inputs(x, cu, cls, wk, bk, heads, out_fmt):
    """(ref64, bound) for a pool call on these operands; empty sequences -> exact zeros."""
    ref, p = reference_pool(x, cu, cls, wk, bk, heads)
    _, lens = _segments(cu)
    ref = torch.where((lens == 0).to(ref.device).view(-1, 1, 1), torch.zeros_like(ref), ref)
    bound, _ = pool_bound(x, cu, cls, wk, heads, ref, p, out_fmt)
    return ref, bound


def mlp_bound(pooled, pooled_bound, w1, b1, w2, b2, fmt):
    """final(relu(linear(pooled))) of the heads, as the package runs it, against float64 on the SAME pooled values: linear on the GEMM
    (bf16: gemm.hip output rounding to bf16 -- the reference's own rounding point after its bf16 nn.Linear; fp32: the split-operand GEMM,
    the pair carries pooled to 2^-16 relative, fp32 result), then esme_hip_relu_linear (fp32 chain, [relu-linear] one rounding to fmt).
    `pooled_bound` propagates the pooling's own bound through both layers.  Returns (ref64 from the exact pooled ref if given, bound)."""
    a = pooled.double()
    if fmt == 'fp32':
        h, hb, _ = gemm_reference(a, w1, b1, out_fmt='fp32')
        hb = hb + (a.abs() * 2.0 ** -16) @ w1.double().abs().T           # the (hi, lo) pair's own rounding of the fp32 pooled value
    else:
        h, hb, _ = gemm_reference(a, w1, b1, out_fmt='bf16')
    hb = hb + pooled_bound.double() @ w1.double().abs().T
    r = torch.relu(h)
    y = r @ w2.double().T + b2.double()
    pre = dot_term(r, w2) + hb @ w2.double().abs().T + U32 * y.abs()
    return y, pre + out_round(y, pre, fmt)


# ------------------------------------------------------------------ CPU emulation of the kernel, with defect switches

def _bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)


def emulate_pool(x, cu, cls, wk, heads, out_dtype, defect=None):
    """float32 emulation of esme_hip_attn_pool_fold + esme_hip_attn_pool.  `defect`: None, 'u_bf16' (U without its lo half),
    'chunk_drop' / 'chunk_repeat' (row R of a chunk dropped / counted twice), 'no_rescale' (combine without the max rescale),
    'scale_d' (1/d instead of 1/sqrt(d)), 'k_as_v' (the projected k used as v), 'neighbour_head' (output column mapped to head + 1),
    'round_twice' (the chunk's output rounded to the output dtype before the combine)."""
    x32 = x.float()
    T, E = x32.shape
    C, H = cls.shape[0], heads
    d = E // H
    scale = torch.tensor(LOG2E / (d if defect == 'scale_d' else math.sqrt(d)), dtype=torch.float32)
    u = torch.einsum('chd,hde->che', cls.float().view(C, H, d), wk.float().view(H, d, E)) * scale
    if defect == 'u_bf16':
        u = _bf16(u)
    V = x32 @ wk.float().T if defect == 'k_as_v' else x32
    cu_l, lens = _segments(cu)
    B = lens.numel()
    out = torch.zeros(B, C, E, dtype=torch.float32)
    for b in range(B):
        a0, n = int(cu_l[b]), int(lens[b])
        if n == 0:
            continue
        ms, ls, os_ = [], [], []
        for r0 in range(0, n, ROWS):
            r1 = min(n, r0 + ROWS)
            rows = list(range(a0 + r0, a0 + r1))
            if defect == 'chunk_drop' and r0 > 0:
                rows = rows[1:]
            if defect == 'chunk_repeat' and r1 < n:
                rows = rows + [a0 + r1]
            xr, vr = x32[rows], V[rows]
            s = torch.einsum('te,che->tch', xr, u)                       # (t, C, H)
            m = s.max(0).values
            p = torch.exp2(s - m)
            l = p.sum(0)
            o = torch.einsum('tch,thd->chd', p, vr.view(-1, H, d)).reshape(C, E)
            if defect == 'round_twice':
                o = o.to(out_dtype).float()
            ms.append(m), ls.append(l), os_.append(o)
        m = torch.stack(ms)                                              # (k, C, H)
        M = m.max(0).values
        a = torch.ones_like(m) if defect == 'no_rescale' else torch.exp2(m - M)
        L = (a * torch.stack(ls)).sum(0)
        O = (a.repeat_interleave(d, dim=2) * torch.stack(os_)).sum(0)
        out[b] = O / L.repeat_interleave(d, dim=1)
    if defect == 'neighbour_head':
        out = out.view(B, C, H, d).roll(1, dims=2).reshape(B, C, E)
    return out.to(out_dtype)
