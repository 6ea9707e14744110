"""float64 restatement, per-element error bound and a CPU emulation for the fused linear + cross-entropy kernel
(csrc/linear_xent.hip, include/esme_hip_linear_xent.h).

`reference` restates the header's definition in float64 on the operands the kernel is handed:
    z = x W^T + b,  lse = logsumexp z,  l_t = cw[y_t] (lse_t - z_{t, y_t}) on kept rows (y_t != ignore_index, 0 <= y_t < C), else 0,
    L = sum l,  D = sum over kept rows of cw[y_t],  loss = L or L / D (0 when D == 0),
    G = g s cw[y_t] (softmax z - onehot y_t) on kept rows, else 0 (s = 1 or 1 / D; 0 when D == 0),  dX = G W, dW = G^T x, db = sum_t G.
`bound` is the sum of the kernel's rounding steps, per element, with the constants of tests/error_bounds.py.  The bf16 inputs are exact
and so are the fp32 products of two of them; a fp32 accumulation of n terms in ANY order is within gamma(n) * sum |terms|,
gamma(n) = n 2^-24 / (1 - n 2^-24):
  [z]     gamma(E + 1) (|x| |W|^T + |b|): the MFMA chain over E and the bias;
  [exp]   per class the argument error carried through exp: [z], the fp32 subtraction z - m and the product with log2 e behind __expf
          (2^-24 |z - m| each), and v_exp_f32 with the allowance tests/attn_bwd_bounds.py uses for exp2f (2 * E_TRANS);
  [lse]   sum_c p_c [exp]_c (the relative error of the row sum), gamma(64) for its additions, v_log_f32 (2 * E_TRANS) and the product
          with ln 2 on |lse - m|, and the addition m + log;
  [l]     cw ([lse] + [z] at y + the subtraction) and the product with cw;
  [L, D]  gamma(T) sum |l| + sum [l];  gamma(T) sum cw;   loss = L / D: first order in both, plus the division;
  [G]     the coefficient g s cw (1 / D: [D] / D and the division; two products), exp(z - lse) with the saved fp32 lse ([z] + [lse] +
          two roundings of the argument + 2 * E_TRANS), the subtraction of the one-hot, the product;
  [bf16]  G is rounded to bfloat16 where it becomes an MFMA operand of dX and dW, and db sums the same rounded values: half a bf16 ulp
          of |G| + [G] (at most 2^-8 |G|, 2^-9 |G| at the top of a binade);
  [acc]   dX: gamma(64) |G| |W| over the padded class tile;  dW: gamma(T) |G|^T |x| (the chunks' fp32 partials, rows in order, and
          their sum in chunk order: T terms in all);  db: gamma(T) sum |G|;
  [out]   one rounding of every output to its type (error_bounds.out_round).
The propagated terms carry 1 % for second-order products, as attn_bwd_bounds.py's do.  No rms floor, no global tolerance.
`emulate` is a float32 / bfloat16 CPU emulation of the stated arithmetic with switches for defects (DEFECTS);
tests/test_linear_xent_cpu.py checks that the bound accepts the faithful emulation and rejects each defect on every case of
tests/test_linear_xent_gpu.py it applies to.  Nothing here is tuned to a GPU run.
"""
import math

import torch

import error_bounds as eb
from error_bounds import E_TRANS, U32

TILE = 64                      # ESME_HIP_LINEAR_XENT_TILE
CHUNK = 512                    # ESME_HIP_LINEAR_XENT_CHUNK
IGNORE = -100
PREFILL = 7.0                  # what the outputs hold before the call in the tests: every element must be overwritten
SECOND_ORDER = 1.01

DEFECTS = ('ignored_in_D', 'cw_missing_D', 'onehot_plus_one', 'no_bias', 'drop_tail', 'pad_softmax', 'drop_chunk', 'no_upstream')
OUTPUTS = ('loss', 'L', 'D', 'loss_rows', 'lse', 'dx', 'dw', 'db')


def _case(name, T, E, C, bias=True, cw=False, mean=True, i64=True, block=None, g=1.0, labels='half'):
    return dict(name=name, T=T, E=E, C=C, bias=bias, cw=cw, mean=mean, i64=i64, block=block, g=g, labels=labels)


# every T of {1, 15, 17, 63, 64, 65, 257, 1000}, E of {64, 320, 1280}, C of {1, 2, 3, 16, 17, 33, 64} at least once; the corners
# T = 65 x C = 17 x E = 320 and T = 1000 x C = 33 x E = 1280; int32 and int64 labels; with and without bias and class weights; mean and
# sum; x as the first / second column block of a (T, 2 E) buffer; about half the rows ignored; out-of-range labels; all rows ignored;
# an upstream gradient of 3
CASES = [
    _case('T1-E64-C3', 1, 64, 3, labels='all'),
    _case('T15-E64-C2-i32-sum', 15, 64, 2, i64=False, mean=False),
    _case('T17-E320-C16-nobias', 17, 320, 16, bias=False),
    _case('T63-E64-C1', 63, 64, 1),
    _case('T64-E64-C64-cw', 64, 64, 64, cw=True),
    _case('T65-E320-C17-cw-block1', 65, 320, 17, cw=True, block=1),
    _case('T65-E320-C17-sum-block0-g3', 65, 320, 17, mean=False, block=0, g=3.0),
    _case('T257-E64-C33-i32-cw-sum', 257, 64, 33, i64=False, cw=True, mean=False),
    _case('T1000-E1280-C33-cw-g3', 1000, 1280, 33, cw=True, g=3.0),
    _case('T1000-E64-C3-nobias-range', 1000, 64, 3, bias=False, labels='range'),
    _case('T257-E320-C64-none-kept', 257, 320, 64, cw=True, labels='none'),
]


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def make_labels(T, C, kind, seed, i64=True):
    """(T,) labels.  'half': about half the rows IGNORE, the last row kept; 'all': every row labelled; 'none': every row ignored
    (IGNORE or out of range); 'range': 'half' with a tenth of the rows -7, C or (int64) 2^31 - 1."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, C, (T,), generator=g, dtype=torch.int64)
    if kind in ('half', 'range'):
        y = torch.where(torch.rand(T, generator=g) < 0.5, torch.full_like(y, IGNORE), y)
        y[T - 1] = (T - 1) % C
    if kind == 'range':
        bad = torch.tensor([-7, C, 2 ** 31 - 1 if i64 else C + 5])
        pick = torch.rand(T, generator=g) < 0.1
        pick[T - 1] = False
        y = torch.where(pick, bad[torch.randint(0, 3, (T,), generator=g)], y)
    if kind == 'none':
        y = torch.where(torch.rand(T, generator=g) < 0.5, torch.full_like(y, IGNORE), torch.full_like(y, C))
    return y if i64 else y.to(torch.int32)


def make_case(case, device='cpu'):
    """The operands of a case as a dict: x (T, E) bf16 (a column block of `buf` (T, 2 E) when case['block'] is set), w (C, E), b (C)
    or None, y, cw (C) float32 or None, g (1,) float32, mean."""
    T, E, C = case['T'], case['E'], case['C']
    seed = 31 + T + 3 * E + 7 * C + len(case['name'])
    g = torch.Generator().manual_seed(seed)
    width = 2 * E if case['block'] is not None else E
    buf = torch.randn(T, width, generator=g).to(torch.bfloat16).to(device)
    x = buf if case['block'] is None else buf[:, case['block'] * E:(case['block'] + 1) * E]
    w = (2.0 * torch.randn(C, E, generator=g) / math.sqrt(E)).to(torch.bfloat16).to(device)
    b = torch.randn(C, generator=g).to(torch.bfloat16).to(device) if case['bias'] else None
    cw = (0.5 + 1.5 * torch.rand(C, generator=g)).float().to(device) if case['cw'] else None
    y = make_labels(T, C, case['labels'], seed + 1, case['i64']).to(device)
    return dict(x=x, buf=buf, w=w, b=b, y=y, cw=cw, g=torch.tensor([case['g']], dtype=torch.float32, device=device), mean=case['mean'])


def _kept(y, C, ignore=IGNORE):
    y = y.long()
    return (y != ignore) & (y >= 0) & (y < C)


def _parts(x, w, b, y, cw, ignore=IGNORE):
    T, C = x.shape[0], w.shape[0]
    x64, w64 = x.double(), w.double()
    b64 = torch.zeros(C, dtype=torch.float64, device=x.device) if b is None else b.double()
    cw64 = torch.ones(C, dtype=torch.float64, device=x.device) if cw is None else cw.double()
    kept = _kept(y, C, ignore)
    ys = torch.where(kept, y.long(), torch.zeros_like(y.long()))
    z = x64 @ w64.T + b64
    lse = torch.logsumexp(z, dim=1)
    zy = z.gather(1, ys.unsqueeze(1)).squeeze(1)
    cwy = torch.where(kept, cw64[ys], torch.zeros_like(lse))
    oh = torch.zeros_like(z).scatter_(1, ys.unsqueeze(1), 1.0) * kept.unsqueeze(1)
    return x64, w64, b64, kept, ys, z, lse, zy, cwy, oh


def reference(x, w, b, y, cw, g, mean, ignore=IGNORE):
    """dict of float64 tensors: loss, L, D, loss_rows (T), lse (T), dx (T, E), dw (C, E), db (C), and G (T, C)."""
    x64, w64, b64, kept, ys, z, lse, zy, cwy, oh = _parts(x, w, b, y, cw, ignore)
    l = torch.where(kept, cwy * (lse - zy), torch.zeros_like(lse))
    L, D = l.sum(), cwy.sum()
    s = (1.0 / D if D != 0 else torch.zeros_like(D)) if mean else torch.ones_like(D)
    loss = L * s if mean else L
    G = float(g.double()) * s * cwy.unsqueeze(1) * (torch.softmax(z, dim=1) - oh) * kept.unsqueeze(1)
    return dict(loss=loss, L=L, D=D, loss_rows=l, lse=lse, dx=G @ w64, dw=G.T @ x64, db=G.sum(0), G=G)


def bound(x, w, b, y, cw, g, mean, ignore=IGNORE, out_fmt='bf16'):
    """dict of float64 bounds for |kernel - reference| of every entry of OUTPUTS (dw / db rounded to `out_fmt`)."""
    x64, w64, b64, kept, ys, z, lse, zy, cwy, oh = _parts(x, w, b, y, cw, ignore)
    ref = reference(x, w, b, y, cw, g, mean, ignore)
    T, E = x.shape
    p = torch.softmax(z, dim=1)
    m = z.max(dim=1, keepdim=True).values
    e_z = gamma(E + 1) * (x64.abs() @ w64.abs().T + b64.abs())                                        # [z]
    eps = e_z + 2 * U32 * (z - m).abs() + 2 * E_TRANS                                                 # [exp]
    e_lse = (p * eps).sum(1) + gamma(64) + (2 * E_TRANS + U32) * (lse - m.squeeze(1)).abs() + U32 * lse.abs()   # [lse]
    e_lse = SECOND_ORDER * e_lse
    e_zy = e_z.gather(1, ys.unsqueeze(1)).squeeze(1)
    l = ref['loss_rows']
    e_l = torch.where(kept, cwy * (e_lse + e_zy + U32 * (lse - zy).abs()) + U32 * l.abs(), torch.zeros_like(l))   # [l]
    e_L = gamma(max(T, 1)) * l.abs().sum() + e_l.sum()                                                # [L, D]
    e_D = gamma(max(T, 1)) * cwy.sum()
    L, D = ref['L'], ref['D']
    if mean:
        e_loss = SECOND_ORDER * (e_L + L.abs() / D * e_D) / D + U32 * ref['loss'].abs() if D != 0 else torch.zeros_like(L)
        rel_coef = (e_D / D if D != 0 else torch.zeros_like(D)) + 3 * U32
    else:
        e_loss, rel_coef = e_L, torch.as_tensor(2 * U32, dtype=torch.float64, device=x.device)
    G = ref['G']
    s = (1.0 / D if D != 0 else torch.zeros_like(D)) if mean else torch.ones_like(D)
    coef = (float(g.double()) * s * cwy).abs().unsqueeze(1)
    eps_p = e_z + e_lse.unsqueeze(1) + 2 * U32 * (z - lse.unsqueeze(1)).abs() + 2 * E_TRANS
    e_G = SECOND_ORDER * (coef * (p * eps_p + U32 * (p - oh).abs()) + G.abs() * (rel_coef + U32)) * kept.unsqueeze(1)   # [G]
    e_Gb = e_G + torch.where(G.abs() + e_G > 0, eb.half_ulp(G.abs() + e_G, 'bf16'), torch.zeros_like(G))                # [bf16]
    pre_dx = e_Gb @ w64.abs() + gamma(64) * (G.abs() @ w64.abs())                                     # [acc]
    pre_dw = e_Gb.T @ x64.abs() + gamma(max(T, 1)) * (G.abs().T @ x64.abs())
    pre_db = e_Gb.sum(0) + gamma(max(T, 1)) * G.abs().sum(0)
    zero = lambda v, pre: torch.where((v == 0) & (pre == 0), torch.zeros_like(pre), pre + eb.out_round(v, pre, 'bf16'))
    zero_o = lambda v, pre: torch.where((v == 0) & (pre == 0), torch.zeros_like(pre), pre + eb.out_round(v, pre, out_fmt))
    return dict(loss=e_loss, L=e_L, D=e_D, loss_rows=e_l, lse=e_lse,
                dx=zero(ref['dx'], pre_dx), dw=zero_o(ref['dw'], pre_dw), db=zero_o(ref['db'], pre_db))     # [out]


def worst(got, ref, bnd):
    """max of err / bound (0 / 0 counts as 0; an error over a zero bound counts as inf)"""
    got = got.detach().double().cpu().reshape(-1)
    ref, bnd = ref.double().cpu().reshape(-1), bnd.double().cpu().reshape(-1)
    assert bool(torch.isfinite(got).all()), 'non-finite output'
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd)
    return float(ratio.max()) if ratio.numel() else 0.0


def worst_of(out, ref, bnd, names=OUTPUTS):
    """{name: worst ratio} over the outputs present in `out`."""
    return {n: worst(out[n], ref[n], bnd[n]) for n in names if out.get(n) is not None}


def defect_applies(defect, case, ops):
    """Whether `defect` changes anything on this case's operands."""
    T, C = case['T'], case['C']
    kept = _kept(ops['y'], C)
    any_kept = bool(kept.any())
    if defect == 'ignored_in_D':
        return case['mean'] and any_kept and not bool(kept.all())
    if defect == 'cw_missing_D':
        return case['mean'] and case['cw'] and any_kept
    if defect == 'onehot_plus_one':
        return any_kept
    if defect == 'no_bias':
        return case['bias'] and any_kept and C > 1
    if defect == 'drop_tail':
        return T % TILE != 0
    if defect == 'pad_softmax':
        return C < 64
    if defect == 'drop_chunk':
        return any_kept and C > 1
    if defect == 'no_upstream':
        return case['g'] != 1.0 and any_kept and C > 1
    raise ValueError(defect)


def _bf(t):
    return t.to(torch.bfloat16).float()


def emulate(x, w, b, y, cw, g, mean, ignore=IGNORE, defect=None):
    """float32 / bfloat16 emulation of esme_hip_linear_xent_fwd and _bwd on the CPU (float64 matrix products stand in for the MFMA's
    fp32 chains over exact products): the dict of OUTPUTS, loss_rows / lse in buffers that held PREFILL.  `defect`: None or one of
    DEFECTS -- 'ignored_in_D' (an ignored row counted in D), 'cw_missing_D' (D counts rows instead of weights), 'onehot_plus_one' (the
    one-hot at class y + 1), 'no_bias' (the bias dropped), 'drop_tail' (the last, partial 64-row tile dropped), 'pad_softmax' (the
    padded classes C .. 63 enter the softmax as zero logits), 'drop_chunk' (the first chunk's dW partial dropped), 'no_upstream' (the
    upstream gradient taken as 1)."""
    assert defect is None or defect in DEFECTS, defect
    x, w, y = x.cpu(), w.cpu(), y.cpu().long()
    T, E = x.shape
    C = w.shape[0]
    b32 = torch.zeros(C) if (b is None or defect == 'no_bias') else b.cpu().float()
    cw32 = torch.ones(C) if cw is None else cw.cpu().float()
    kept = _kept(y, C, ignore)
    live = torch.ones(T, dtype=torch.bool)
    if defect == 'drop_tail' and T % TILE:
        live[T // TILE * TILE:] = False
    kept = kept & live
    ys = torch.where(kept, y, torch.zeros_like(y))
    z = (x.double() @ w.double().T).float() + b32                                     # [z]
    m = z.max(dim=1, keepdim=True).values
    if defect == 'pad_softmax' and C < 64:
        m = torch.clamp(m, min=0.0)
    e = torch.exp(z - m).sum(1)
    if defect == 'pad_softmax' and C < 64:
        e = e + (64 - C) * torch.exp(-m.squeeze(1))
    lse = m.squeeze(1) + torch.log(e)                                                 # [lse]
    zy = z.gather(1, ys.unsqueeze(1)).squeeze(1)
    cwy = torch.where(kept, cw32[ys], torch.zeros(T))
    l = torch.where(kept, cwy * (lse - zy), torch.zeros(T))                           # [l]
    d_rows = cwy.clone()
    if defect == 'cw_missing_D':
        d_rows = kept.float()
    if defect == 'ignored_in_D':
        d_rows = torch.where(kept, d_rows, torch.ones(T)) * live
    n_tiles = -(-T // TILE)
    L = torch.zeros((), dtype=torch.float32)
    D = torch.zeros((), dtype=torch.float32)
    for t in range(n_tiles):                                                          # [L, D] tile partials, then their sum
        sl = slice(t * TILE, min(T, (t + 1) * TILE))
        L = L + l[sl].sum()
        D = D + d_rows[sl].sum()
    loss = (L / D if D != 0 else torch.zeros(())) if mean else L
    gv = 1.0 if defect == 'no_upstream' else float(g)
    s = (torch.tensor(1.0) / D if D != 0 else torch.zeros(())) if mean else torch.ones(())
    coef = (torch.tensor(gv, dtype=torch.float32) * s) * cwy
    hot = ys + 1 if defect == 'onehot_plus_one' else ys
    oh = torch.zeros(T, C + 1).scatter_(1, hot.unsqueeze(1), 1.0)[:, :C]
    G = coef.unsqueeze(1) * (torch.exp(z - lse.unsqueeze(1)) - oh) * kept.unsqueeze(1)            # [G]
    Gb = _bf(G)                                                                       # [bf16]
    dx = (Gb.double() @ w.double()).float().to(torch.bfloat16)
    dw = torch.zeros(C, E, dtype=torch.float32)
    for c in range(-(-T // CHUNK)):                                                   # [acc] chunk partials, in chunk order
        if defect == 'drop_chunk' and c == 0:
            continue
        sl = slice(c * CHUNK, min(T, (c + 1) * CHUNK))
        dw = dw + (Gb[sl].double().T @ x[sl].double()).float()
    db = torch.zeros(C, dtype=torch.float32)
    for t in range(n_tiles):
        db = db + Gb[t * TILE:(t + 1) * TILE].sum(0)
    loss_rows = torch.where(live, l, torch.full((T,), PREFILL))
    lse_out = torch.where(live, lse, torch.full((T,), PREFILL))
    return dict(loss=loss, L=L, D=D, loss_rows=loss_rows, lse=lse_out, dx=dx, dw=dw.to(torch.bfloat16),
                db=db.to(torch.bfloat16) if b is not None else None)
