"""float64 reference, per-element error bound and a CPU emulation for the token-embedding gradient (csrc/embed_bwd.hip).

`reference` is dE[v] = the sum of the rows of dX whose id is v (v not excluded, ids outside [0, V) dropped) in float64 on the operands
the kernel is handed.  `bound` is the sum of the kernel's rounding steps, built from tests/error_bounds.py's constants:
 1. the fp32 accumulation of the n_vc rows of id v inside chunk c, in the statistical form C_DOT * U32 * sqrt(n_vc) * ||dX[rows, e]||_2
    (error_bounds.C_DOT covers sequential fp32 accumulation; the summands are exact bf16 values);
 2. the ordered fp32 sum of the chunks' partials: chunks - 1 adds, each within U32 of the running magnitude, bounded by
    (chunks - 1) * U32 * sum_c |partial_c|;
 3. one rounding to bfloat16 (error_bounds.out_round).
A row of an id that does not occur or is excluded has bound 0 up to the subnormal floor: it must be exact zeros.
`emulate` is a float32 CPU emulation of the kernel's order (rows ascending inside a chunk of ROWS rows, chunks ascending, one
rounding) with switches for defects; tests/test_embed_bwd_cpu.py checks that the bound accepts the faithful emulation and rejects each
defect on the cases tests/test_embed_bwd_gpu.py runs.  Nothing here is tuned to a GPU run.
"""
import math

import torch

import error_bounds as eb

ROWS = 256                     # ESME_HIP_EMBED_BWD_ROWS (include/esme_hip_embed_bwd.h)
PREFILL = 7.0                  # what dE holds before the call in the tests: every element must be overwritten
ABSENT = 3                     # an id `make_tokens` never draws
DEFECTS = ('count_mask', 'count_pad', 'drop_tail', 'id_plus_one', 'wrap_ids', 'bf16_acc', 'absent_unwritten')

TS = (1, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 1, 2051)
ES = (64, 320)
VS = (33, 64)
# (name, T, E, V, kind of ids, mask_idx, pad_idx); mask_idx = V - 1 and pad_idx = 1 are ESM-2's positions in a table of 33 rows
GRID = [(f'T{T}-E{E}-V{V}', T, E, V, 'skew', V - 1, 1) for T in TS for E in ES for V in VS]
EXTRA = [('one-id', 2051, 64, 33, 'one', 32, 1),                # all rows one id: a fan-in of 2 051 (the bf16-accumulation defect shows here)
         ('out-of-range', 300, 64, 33, 'range', 32, 1),         # a tenth of the ids is -1 or V
         ('no-exclusion', 2 * ROWS + 1, 64, 33, 'skew', -1, -1),  # mask_idx = pad_idx = -1: the <mask> and <pad> rows train (ESM-C's <mask>)
         ('no-exclusion-V64', ROWS + 1, 320, 64, 'skew', -1, -1)]
CASES = GRID + EXTRA


def make_tokens(T, V, kind, seed, mask_idx, pad_idx):
    """int64 (T,).  'skew': a proteome-like skew (frequency ~ 1 / rank over a shuffled table, so the commonest id holds about a
    quarter of the rows and most ids are rare), never ABSENT; from T >= 8 on one row each of the <mask> id V - 1, the <pad> id 1, -1
    and V.  'one': every row id 5.  'range': 'skew' with a tenth of the rows -1 or V."""
    g = torch.Generator().manual_seed(seed)
    if kind == 'one':
        return torch.full((T,), 5, dtype=torch.int64)
    order = torch.randperm(V, generator=g)
    w = torch.zeros(V, dtype=torch.float64)
    w[order] = 1.0 / torch.arange(1, V + 1, dtype=torch.float64)
    w[ABSENT] = 0.0
    if T < 8:
        w[[1, V - 1]] = 0.0                                       # (a single row is an ordinary id)
    tok = torch.multinomial(w, T, replacement=True, generator=g)
    if T >= 8:
        tok[1], tok[2], tok[3], tok[4] = V - 1, 1, -1, V
        tok[T - 1] = 5                                            # the last (partial) chunk holds a row that counts
    if kind == 'range':
        bad = torch.rand(T, generator=g) < 0.1
        tok = torch.where(bad, torch.where(torch.rand(T, generator=g) < 0.5, torch.tensor(-1), torch.tensor(V)), tok)
    return tok


def make_dx(T, E, seed, pad=24, device='cpu'):
    """dX (T, E) bfloat16 as a column view (first column 8) of a buffer with row stride E + pad, and the buffer."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(T, E + pad, generator=g).to(torch.bfloat16).to(device)
    return buf[:, 8:8 + E], buf


def make_case(case, device='cpu'):
    name, T, E, V, kind, mask_idx, pad_idx = case
    seed = 11 + T + 3 * E + 7 * V + len(name)
    dx, buf = make_dx(T, E, seed, device=device)
    return dx, make_tokens(T, V, kind, seed + 1, mask_idx, pad_idx).to(device)


def _valid(tok, V, mask_idx, pad_idx):
    return (tok >= 0) & (tok < V) & (tok != mask_idx) & (tok != pad_idx)


def reference(dx, tok, V, mask_idx, pad_idx):
    """dE (V, E) float64."""
    ok = _valid(tok, V, mask_idx, pad_idx)
    ref = torch.zeros(V, dx.shape[1], dtype=torch.float64, device=dx.device)
    return ref.index_add_(0, tok[ok], dx.double()[ok])


def bound(dx, tok, V, mask_idx, pad_idx):
    """(bound, pre) float64 (V, E) for |kernel - reference|; `pre` is the bound before the output rounding."""
    T, E = dx.shape
    chunks = -(-T // ROWS)
    ok = _valid(tok, V, mask_idx, pad_idx)
    dx64 = dx.double()
    pre = torch.zeros(V, E, dtype=torch.float64, device=dx.device)
    mag = torch.zeros_like(pre)
    for c in range(chunks):
        sl = slice(c * ROWS, min(T, (c + 1) * ROWS))
        t, o, x = tok[sl], ok[sl], dx64[sl]
        n = torch.zeros(V, dtype=torch.float64, device=dx.device).index_add_(0, t[o], torch.ones(int(o.sum()), dtype=torch.float64, device=dx.device))
        ss = torch.zeros_like(pre).index_add_(0, t[o], x[o] * x[o])
        pre += eb.C_DOT * eb.U32 * torch.sqrt(n).unsqueeze(1) * torch.sqrt(ss)          # 1. the chunk's fp32 chain, rows in order
        mag += torch.zeros_like(pre).index_add_(0, t[o], x[o]).abs()
    pre += max(chunks - 1, 0) * eb.U32 * mag                                            # 2. the chunks' partials, in chunk order
    ref = reference(dx, tok, V, mask_idx, pad_idx)
    return pre + eb.out_round(ref, pre, 'bf16'), pre                                    # 3. one rounding to bfloat16


def worst(got, ref, bnd):
    """max of err / bound (0 / 0 counts as 0)"""
    assert bool(torch.isfinite(got.double()).all()), 'non-finite output'
    err = (got.double() - ref.to(got.device)).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd.to(got.device))
    return float(ratio.max()) if ratio.numel() else 0.0


def defect_applies(defect, tok, V, mask_idx, pad_idx):
    """Whether `defect` changes anything on these ids."""
    T = tok.numel()
    ok = _valid(tok, V, mask_idx, pad_idx)
    if defect == 'count_mask':
        return mask_idx >= 0 and bool((tok == mask_idx).any())
    if defect == 'count_pad':
        return pad_idx >= 0 and bool((tok == pad_idx).any())
    if defect == 'drop_tail':
        return T % ROWS != 0 and bool(ok[T // ROWS * ROWS:].any())
    if defect == 'id_plus_one':
        return bool(ok.any())
    if defect == 'wrap_ids':
        out = tok[(tok < 0) | (tok >= V)] % V
        return bool(((out != mask_idx) & (out != pad_idx)).any())
    if defect == 'bf16_acc':                                     # (the rounding of a long chain: one id with about 1 000 rows or more)
        return bool(ok.any()) and int(torch.bincount(tok[ok], minlength=V).max()) >= 1000
    if defect == 'absent_unwritten':
        return T > 0 and int(torch.bincount(tok[(tok >= 0) & (tok < V)], minlength=V).min()) == 0
    raise ValueError(defect)


def emulate(dx, tok, V, mask_idx, pad_idx, defect=None):
    """float32 emulation of esme_hip_embed_bwd on the CPU: dE (V, E) bfloat16 in a table that held PREFILL.  `defect`: None or one of
    DEFECTS -- 'count_mask' / 'count_pad' (the rows of the excluded id summed like any other), 'drop_tail' (the last, partial chunk
    dropped), 'id_plus_one' (every row lands one table row further down), 'wrap_ids' (an id outside [0, V) taken modulo V),
    'bf16_acc' (the accumulators rounded to bfloat16 after every add), 'absent_unwritten' (the row of an id that does not occur is
    left as it was)."""
    assert defect is None or defect in DEFECTS, defect
    T, E = dx.shape
    x32, ids = dx.float().cpu(), tok.cpu().tolist()
    chunks = -(-T // ROWS)
    if defect == 'drop_tail' and T % ROWS:
        chunks -= 1
    m = -1 if defect == 'count_mask' else mask_idx
    p = -1 if defect == 'count_pad' else pad_idx
    total = torch.zeros(V, E, dtype=torch.float32)
    for c in range(chunks):
        acc = torch.zeros(V, E, dtype=torch.float32)
        for t in range(c * ROWS, min(T, (c + 1) * ROWS)):                               # rows in ascending order
            v = ids[t]
            if defect == 'wrap_ids':
                v %= V
            if defect == 'id_plus_one':
                v += 1
            if 0 <= v < V and v != m and v != p:
                acc[v] += x32[t]
                if defect == 'bf16_acc':
                    acc[v] = acc[v].to(torch.bfloat16).float()
        total = total + acc                                                             # chunks in ascending order
    out = total.to(torch.bfloat16)
    if defect == 'absent_unwritten':
        seen = torch.bincount(tok.cpu()[(tok.cpu() >= 0) & (tok.cpu() < V)], minlength=V) > 0
        out[~seen] = PREFILL
    return out
