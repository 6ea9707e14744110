"""float64 reference, per-element error bounds and a CPU emulation for the attention-pooling backward (csrc/pool_bwd.hip).

`reference_pool_grads` is float64 autograd through the folded definition the kernel differentiates (include/esme_hip_attn_pool_bwd.h):
sigma = U x, p = 2^sigma normalised over each sequence's rows, out = sum_t p x -- on the operands the kernel is handed, x as stored and
U as the fp32 tensor.  `pool_bwd_bound` is the sum of the kernel's rounding steps, each tagged with the marker of the kernel line that
performs it ([score], [dp], ...), built from tests/error_bounds.py's constants and `dot_term`, in the style of attn_pool_bounds.py.
`emulate_pool_bwd` is a float32 CPU emulation of the kernel's order of operations with switches for defects;
tests/test_attn_pool_bwd_cpu.py checks that the bound accepts the correct emulation and rejects each defect, on the shapes
tests/test_attn_pool_bwd_gpu.py runs.  Nothing here is tuned to a GPU run.
"""
import math

import torch

from error_bounds import C_DOT, E_TRANS, U32, dot_term, out_round

ROWS = 64                   # kPoolRows: rows per chunk (pool.h)
LN2 = math.log(2.0)

EDGES = (0, 1, 2, 63, 64, 65, 129, 0, 200)
SHAPES = [                  # (lengths, E, H, n_cls): the smallest shapes at which the kernel can go wrong
    (EDGES, 64, 4, 1),      # empty sequences; chunk boundaries
    (EDGES, 64, 4, 3),      # several class tokens
    ((5, 70), 40, 5, 2),    # d = 8; E not a multiple of the 32-column slab
    ((3, 66), 64, 8, 9),    # J = 72, past one 64-column score pass
]
DEFECTS = ('no_ln2', 'no_delta', 'delta_bf16_out', 'chunk_stats', 'no_value_path', 'dp_head_shift', 'row_twice', 'skip_last_partial')


def cu_of(lengths):
    cu = torch.zeros(len(lengths) + 1, dtype=torch.int32)
    cu[1:] = torch.tensor(lengths).cumsum(0)
    return cu


def make_operands(lengths, E, H, C, dtype, seed, device='cpu'):
    """x (T, E) and d_out (B, C, E) in `dtype`, U (C H, E) fp32 with scores sigma = U x of standard deviation ~1.4 (log2 units: natural
    scores of about 1), cu_lens int32."""
    g = torch.Generator().manual_seed(seed)
    T, B = sum(lengths), len(lengths)
    x = torch.randn(T, E, generator=g).to(dtype)
    U = (torch.randn(C * H, E, generator=g) * (1.4426950408889634 / math.sqrt(E))).float()
    d_out = torch.randn(B, C, E, generator=g).to(dtype)
    return dict(x=x.to(device), U=U.to(device), d_out=d_out.to(device), cu=cu_of(lengths).to(device), heads=H, n_cls=C)


def _segments(cu):
    cu = cu.to(torch.long).cpu()
    return cu, cu[1:] - cu[:-1]


def _forward64(x64, cu, U64, heads):
    """(out (B, C, E), p (T, J)) float64 of the folded definition; differentiable."""
    T, E = x64.shape
    J = U64.shape[0]
    H, C, d = heads, J // heads, E // heads
    cu_l, lens = _segments(cu)
    outs, ps = [], []
    for b in range(lens.numel()):
        a, n = int(cu_l[b]), int(lens[b])
        if n == 0:
            outs.append(torch.zeros(C, E, dtype=torch.float64, device=x64.device))
            continue
        xs = x64[a:a + n]
        p = torch.softmax(LN2 * (xs @ U64.T), dim=0)                    # 2^sigma normalised over the sequence's rows
        outs.append(torch.einsum('tch,thd->chd', p.view(n, C, H), xs.view(n, H, d)).reshape(C, E))
        ps.append(p)
    p_all = torch.cat(ps) if ps else torch.zeros(0, J, dtype=torch.float64, device=x64.device)
    return torch.stack(outs), p_all


def reference_pool_grads(x, cu, U, d_out, heads):
    """(dX (T, E), dU (J, E)) float64: autograd through the folded definition on the operands the kernel is handed."""
    x64 = x.detach().double().requires_grad_()
    U64 = U.detach().double().requires_grad_()
    out, _ = _forward64(x64, cu, U64, heads)
    if x64.numel() == 0 or not out.requires_grad:
        return torch.zeros_like(x64), torch.zeros_like(U64)
    out.backward(d_out.double())
    return x64.grad, (U64.grad if U64.grad is not None else torch.zeros_like(U64))


def pool_bwd_bound(x, cu, U, d_out, heads, ref_dx, out_fmt):
    """(bound of dX (T, E), bound of dU (J, E)) float64 for |kernel - reference_pool_grads|.  `out_fmt`: the dtype of dX ('bf16' /
    'fp32'); dU is fp32 and carries its accumulation terms only."""
    x64, U64, g64 = x.double(), U.double(), d_out.double()
    T, E = x64.shape
    J = U64.shape[0]
    H, C, d = heads, J // heads, E // heads
    dev = x64.device
    cu_l, lens = _segments(cu)
    B = lens.numel()
    seg = torch.repeat_interleave(torch.arange(B, device=dev), lens.to(dev))
    if T == 0:
        return torch.zeros(T, E, dtype=torch.float64, device=dev), torch.zeros(J, E, dtype=torch.float64, device=dev)
    idx = seg.view(-1, 1).expand(T, J)

    def seg_sum(v):                                                      # (T, J) -> (B, J)
        return torch.zeros(B, J, dtype=torch.float64, device=dev).index_add_(0, seg, v)

    def seg_max(v):
        return torch.zeros(B, J, dtype=torch.float64, device=dev).scatter_reduce(0, idx, v, 'amax')

    _, p = _forward64(x64, cu, U64, heads)
    s = x64 @ U64.T                                                      # (T, J), log2 units
    # [score] fp32 fmaf chain over E products U_e x_e
    ds = dot_term(x64, U64)
    # relative error of an unnormalised weight 2^(sigma - max): its score error and the max row's, the fp32 subtractions sigma - m
    # ([chunk-exp], [p-exp]) and m_k - M ([stat-exp]) (|.| <= |s| + 3 max|s|), one v_exp_f32 in each of the (at most) two steps
    eps = LN2 * (ds + seg_max(ds)[seg] + U32 * (s.abs() + 3 * seg_max(s.abs())[seg])) + 2 * E_TRANS
    nr = torch.clamp(lens, max=ROWS).to(dev).double()
    nch = torch.div(lens + ROWS - 1, ROWS, rounding_mode='floor').to(dev).double()
    n_acc = (nr + nch).view(B, 1)                                        # [chunk-sum] / [chunk-delta] <= 64 terms, [stat-sum] / [stat-delta] one fmaf per chunk
    # the normaliser: every term with its weight's error, the two chains; [inv-l] and [p-norm] one rounding each
    eps_p = eps + (seg_sum(p * eps) + (n_acc + 2) * U32)[seg]            # relative error of p_tj
    # [dp] fp32 fmaf chain over d products dO_i x_i
    gh, xh = g64.view(B, C, H, d), x64.view(T, H, d)
    dP = torch.einsum('thd,tchd->tch', xh, gh[seg]).reshape(T, J)
    ddP = C_DOT * U32 * math.sqrt(d) * torch.sqrt(torch.einsum('thd,tchd->tch', xh * xh, (gh * gh)[seg])).reshape(T, J)
    delta = seg_sum(p * dP)
    # [chunk-delta] [stat-delta] [delta]: Delta = sum_t p_t dP_t with the weights of the chunk path, the two chains and the product with 1 / l
    ddelta = seg_sum(p * (dP.abs() * (eps_p + (n_acc[seg] + 1) * U32) + ddP))
    diff = dP - delta[seg]
    dsig = LN2 * p * diff
    # [dsigma] ln2 (a constant rounded to fp32) * p * (dP - Delta): the subtraction and two products
    ddsig = LN2 * p * (ddP + ddelta[seg] + diff.abs() * (eps_p + 4 * U32))
    # ---- dU: [du-chunk] the chunk's fmaf chain in row order, [du-sum] the partials in slot order: one accumulation over the T rows
    bU = ddsig.T @ x64.abs() + dot_term(dsig.T, x64.T)
    bU = 1.01 * bU                                                       # 1 %: the second-order terms of the first-order sums above
    # ---- dX: [dx-score] fmaf chain over j, [dx-value] over c: J + C terms (linear form); the value path's p has eps_p
    jc = (torch.arange(C, device=dev).view(C, 1) * H + torch.arange(E, device=dev).view(1, E) // d)        # (C, E): j of (c, h(e))
    pv = p[:, jc]                                                        # (T, C, E)
    gv = g64[seg]                                                        # (T, C, E)
    mag = dsig.abs() @ U64.abs() + (pv * gv.abs()).sum(1)
    pre = ddsig @ U64.abs() + (eps_p[:, jc] * pv * gv.abs()).sum(1) + (J + C) * U32 * mag
    pre = 1.01 * pre
    # [dx-round] one rounding to the output dtype
    bX = pre + out_round(ref_dx, pre, out_fmt)
    return bX, bU


def worst(got, ref, bound):
    """max over (dX, dU) of err / bound (0 / 0 counts as 0; a non-zero error on a zero bound as inf)"""
    w = 0.0
    for g, r, b in zip(got, ref, bound):
        if g.numel() == 0:
            continue
        err = (g.double() - r.double()).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / b.double())
        w = max(w, float(ratio.max()))
    return w


# ------------------------------------------------------------------ CPU emulation of the kernel, with defect switches

def emulate_pool_bwd(x, cu, U, d_out, heads, defect=None, need_dx=True):
    """float32 emulation of esme_hip_attn_pool_bwd: (dX in x's dtype or None, dU fp32).  `defect`: None or one of DEFECTS --
    'no_ln2' (ln 2 dropped from dsigma), 'no_delta' (Delta dropped), 'delta_bf16_out' (Delta = dO . out with out rounded to bf16),
    'chunk_stats' (each chunk normalised with its own max / sum / Delta), 'no_value_path' (sum_c p dO dropped from dX),
    'dp_head_shift' (dP of head h from dO's slice of head h - 1), 'row_twice' (the row after a chunk's last counted in that chunk too),
    'skip_last_partial' (the last slot's partial left out of dU)."""
    assert defect is None or defect in DEFECTS, defect
    x32, U32_, g32 = x.float(), U.float(), d_out.float()
    T, E = x32.shape
    J = U32_.shape[0]
    H, C, d = heads, J // heads, E // heads
    cu_l, lens = _segments(cu)
    dX = torch.zeros(T, E, dtype=torch.float32)
    parts = []
    ln2 = torch.tensor(1.0 if defect == 'no_ln2' else LN2, dtype=torch.float32)
    for b in range(lens.numel()):
        a0, n = int(cu_l[b]), int(lens[b])
        if n == 0:
            continue
        gh = g32[b].view(C, H, d)
        ghp = gh.roll(1, dims=1) if defect == 'dp_head_shift' else gh
        chunks = []
        for r0 in range(0, n, ROWS):
            r1 = min(n, r0 + ROWS)
            rows = list(range(a0 + r0, a0 + r1))
            own = len(rows)
            if defect == 'row_twice' and r1 < n:
                rows = rows + [a0 + r1]
            xr = x32[rows]
            s = xr @ U32_.T                                              # [score]
            dP = torch.einsum('thd,chd->tch', xr.view(-1, H, d), ghp).reshape(-1, J)      # [dp]
            m = s.max(0).values
            w = torch.exp2(s - m)                                        # [chunk-exp]
            chunks.append(dict(rows=rows, own=own, x=xr, s=s, dP=dP, m=m, l=w.sum(0), dl=(w * dP).sum(0)))
        m = torch.stack([c['m'] for c in chunks])
        M = m.max(0).values
        a = torch.exp2(m - M)                                            # [stat-exp]
        il = 1.0 / (a * torch.stack([c['l'] for c in chunks])).sum(0)    # [stat-sum] [inv-l]
        delta = (a * torch.stack([c['dl'] for c in chunks])).sum(0) * il                  # [stat-delta] [delta]
        if defect == 'delta_bf16_out':
            out = torch.zeros(C, H, d)
            for c in chunks:
                p = torch.exp2(c['s'] - M) * il
                out += torch.einsum('tch,thd->chd', p.view(-1, C, H), c['x'].view(-1, H, d))
            delta = (gh * out.to(torch.bfloat16).float()).sum(-1).reshape(J)
        if defect == 'no_delta':
            delta = torch.zeros(J)
        for c in chunks:
            Mk, ilk, dk = M, il, delta
            if defect == 'chunk_stats':
                Mk, ilk = c['m'], 1.0 / c['l']
                dk = c['dl'] * ilk
            p = torch.exp2(c['s'] - Mk) * ilk                            # [p-exp] [p-norm]
            dsig = ln2 * p * (c['dP'] - dk)                              # [dsigma]
            parts.append(dsig.T @ c['x'])                                # [du-chunk]
            if need_dx:
                own = c['own']
                v = dsig[:own] @ U32_                                    # [dx-score]
                if defect != 'no_value_path':
                    pe = p[:own].view(own, C, H).repeat_interleave(d, dim=2)              # (t, C, E): p of (c, h(e))
                    v = v + (pe * g32[b]).sum(1)                         # [dx-value]
                dX[c['rows'][:own]] = v
    if defect == 'skip_last_partial':
        parts = parts[:-1]
    dU = torch.zeros(J, E, dtype=torch.float32)
    for part in parts:                                                   # [du-sum] slot order
        dU = dU + part
    return (dX.to(x.dtype) if need_dx else None), dU                     # [dx-round]
