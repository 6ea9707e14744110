"""float64 reference, per-element error bound and a CPU emulation for the position-table gradient (csrc/embed_positions_bwd.hip).

`reference` is dP[p + pos_offset] = the sum over the sequences b with len_b > p of dX[cu_lens[b] + p], p < max_len, in float64 on the
operands the kernel is handed; every other row of the (P, E) table is zero.  `bound` is the sum of the kernel's rounding steps in the
order include/esme_hip_embed_positions_bwd.h states (sequences ascending, fp32 accumulators that start at +0.0, one rounding):
 1. the first add, 0 + x, is exact (x is a bf16 value); every later add of the running sum rounds once, within U32 of the sum's
    magnitude: with S_k the exact partial sum after k sequences and e_k the error so far,  e_k = e_(k-1) + U32 (|S_k| + e_(k-1)),
    e_1 = 0 -- a worst-case bound, not a statistical one (the fan-in is small);
 2. one rounding to bfloat16 (error_bounds.out_round).
No rms floor.  A row no sequence reaches has bound 0 up to the subnormal floor: it must be exact zeros.
`emulate` is the same order in torch float32 on the CPU (a sequence too short for a row adds nothing, as in the kernel), with switches
for defects; tests/test_embed_positions_bwd_cpu.py checks that the bound accepts the faithful emulation and rejects each defect on
the cases tests/test_embed_positions_bwd_gpu.py runs.  A summation in descending sequence order is NOT among the defects: in honest
fp32 it stays inside any bound of this kind; the GPU test's bit-equality with `emulate` is what pins the order.  Nothing here is tuned
to a GPU run.
"""
import torch

import error_bounds as eb

PREFILL = 7.0                  # what dP holds before the call in the tests: every element must be overwritten
TAIL = 3                       # rows of dX behind the last sequence (cu_lens[B] < T): they belong to nobody
LD32 = 1 << 28                 # the row stride the 'offsets32' defect pretends dX has: row 8 starts at element 2^31
DEFECTS = ('bf16_acc', 'offset_plus_one', 'drop_last', 'len_ge', 'past_max_len_unwritten', 'offsets32')

ES = (64, 320)                 # 8 and 40 column groups per table row: at 40 a wave of 64 work items straddles table rows
PATTERNS = {
    'one': (5,),
    'ones': (1, 1, 1),
    'empties': (0, 7, 0, 3),                                     # empty sequences first and in the middle
    'mixed': (33, 1, 64, 2, 65),
    'b65': tuple(1 + (7 * b) % 70 for b in range(65)),
    'fan300': (3,) * 300,                                        # a fan-in of 300 on three rows
}
# (name, E, lens, P - (max_len + pos_offset), pos_offset, max_len); max_len None: the longest sequence
GRID = [(f'{n}-E{E}-P+{extra}', E, lens, extra, 2, None) for n, lens in PATTERNS.items() for E in ES for extra in (0, 38)]
EXTRA = [('mixed-E64-offset0', 64, PATTERNS['mixed'], 0, 0, None),       # pos_offset = 0
         ('b65-E320-clipped', 320, PATTERNS['b65'], 38, 2, 20)]          # max_len below the longest sequence: only the first 20 rows of each
CASES = GRID + EXTRA


def params(case):
    """(E, cu_lens list, T, P, pos_offset, max_len) of a case."""
    name, E, lens, extra, off, max_len = case
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    max_len = max(lens) if max_len is None else max_len
    return E, cu, cu[-1] + TAIL, max_len + off + extra, off, max_len


def make_dx(T, E, seed, pad=24, device='cpu'):
    """dX (T, E) bfloat16 as a column view (first column 8) of a buffer with row stride E + pad, and the buffer."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(T, E + pad, generator=g).to(torch.bfloat16).to(device)
    return buf[:, 8:8 + E], buf


def make_case(case, device='cpu'):
    """(dx, cu_lens int32, P, pos_offset, max_len)"""
    E, cu, T, P, off, max_len = params(case)
    dx, _ = make_dx(T, E, 23 + T + 3 * E + 5 * P + len(case[0]), device=device)
    return dx, torch.tensor(cu, dtype=torch.int32, device=device), P, off, max_len


def _walk(cu_lens, max_len):
    """(b, start, n) for the sequences in ascending order: n = the rows of sequence b that are summed."""
    cu = [int(c) for c in cu_lens.tolist()]
    return [(b, cu[b], min(cu[b + 1] - cu[b], max_len)) for b in range(len(cu) - 1)]


def _by_position(cu_lens, max_len):
    """(p, the rows of dX summed into position p, in the kernel's order) for every position some sequence reaches: the other way
    round the same sums, for a batch of many short sequences (70 002 sequences are three positions, not 70 002 slices)."""
    cu = cu_lens.to(torch.int64).cpu()
    lens = cu[1:] - cu[:-1]
    for p in range(min(max_len, int(lens.max()) if lens.numel() else 0)):
        yield p, cu[:-1][lens > p] + p


def _many(cu_lens, max_len):
    return cu_lens.numel() - 1 > 4 * max_len


def reference(dx, cu_lens, P, pos_offset, max_len):
    """dP (P, E) float64."""
    ref = torch.zeros(P, dx.shape[1], dtype=torch.float64, device=dx.device)
    if _many(cu_lens, max_len):
        for p, rows in _by_position(cu_lens, max_len):
            ref[pos_offset + p] = dx[rows.to(dx.device)].double().sum(0)
        return ref
    x = dx.double()
    for b, s, n in _walk(cu_lens, max_len):
        ref[pos_offset:pos_offset + n] += x[s:s + n]
    return ref


def fan_in(cu_lens, P, pos_offset, max_len):
    """(P,) how many sequences reach each table row."""
    cnt = torch.zeros(P, dtype=torch.int64)
    for b, s, n in _walk(cu_lens, max_len):
        cnt[pos_offset:pos_offset + n] += 1
    return cnt


def bound(dx, cu_lens, P, pos_offset, max_len):
    """(bound, pre) float64 (P, E) for |kernel - reference|; `pre` is the bound before the output rounding."""
    E = dx.shape[1]
    S = torch.zeros(P, E, dtype=torch.float64, device=dx.device)
    pre = torch.zeros_like(S)
    if _many(cu_lens, max_len):                                                         # the recurrence in closed form, per position:
        for p, rows in _by_position(cu_lens, max_len):                                  # e_n = sum over k = 2 .. n of U32 |S_k| (1 + U32)^(n - k)
            part = dx[rows.to(dx.device)].double().cumsum(0)
            n = part.shape[0]
            w = (1.0 + eb.U32) ** torch.arange(n - 1, -1, -1, dtype=torch.float64, device=dx.device)
            w[0] = 0.0                                                                  # 1. the first add is exact
            S[pos_offset + p] = part[-1]
            pre[pos_offset + p] = eb.U32 * (w.unsqueeze(1) * part.abs()).sum(0)
        return pre + eb.out_round(S, pre, 'bf16'), pre
    cnt = torch.zeros(P, dtype=torch.int64, device=dx.device)
    x = dx.double()
    for b, s, n in _walk(cu_lens, max_len):
        rows = slice(pos_offset, pos_offset + n)
        S[rows] += x[s:s + n]
        cnt[rows] += 1
        later = (cnt[rows] >= 2).unsqueeze(1).double()                                  # 1. the first add is exact, every later one rounds once
        pre[rows] += later * eb.U32 * (S[rows].abs() + pre[rows])
    return pre + eb.out_round(S, pre, 'bf16'), pre                                      # 2. one rounding to bfloat16


def worst(got, ref, bnd):
    """max of err / bound (0 / 0 counts as 0)"""
    assert bool(torch.isfinite(got.double()).all()), 'non-finite output'
    err = (got.double() - ref.to(got.device)).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd.to(got.device))
    return float(ratio.max()) if ratio.numel() else 0.0


def dead_rows(cu_lens, P, pos_offset, max_len):
    """bool (P,): the rows that must be exact zeros (below pos_offset, from pos_offset + max_len on, reached by no sequence)."""
    return fan_in(cu_lens, P, pos_offset, max_len) == 0


def defect_applies(defect, case):
    """Whether `defect` changes anything on this case."""
    E, cu, T, P, off, max_len = params(case)
    lens = [b - a for a, b in zip(cu[:-1], cu[1:])]
    if defect == 'bf16_acc':                                     # (the rounding of a long chain: a fan-in of 60 or more)
        return int(fan_in(torch.tensor(cu), P, off, max_len).max()) >= 60
    if defect in ('offset_plus_one', 'drop_last'):
        return any(n > 0 for n in lens)
    if defect == 'len_ge':                                       # a sequence that ends below max_len has a row behind it (TAIL > 0)
        return any(n < max_len for n in lens)
    if defect == 'past_max_len_unwritten':
        return P > max_len + off
    if defect == 'offsets32':                                    # a summed row at index 8 or beyond
        return any(s + n > 8 for s, n in zip(cu[:-1], (min(n, max_len) for n in lens)) if n > 0)
    raise ValueError(defect)


def emulate(dx, cu_lens, P, pos_offset, max_len, defect=None):
    """float32 emulation of esme_hip_embed_positions_bwd on the CPU: dP (P, E) bfloat16 in a table that held PREFILL.  `defect`: None or
    one of DEFECTS -- 'bf16_acc' (the accumulators rounded to bfloat16 after every add), 'offset_plus_one' (every row lands one table
    row further down; the last one is lost where the table ends), 'drop_last' (the last row of each sequence dropped), 'len_ge'
    (len_b >= p in place of len_b > p: the row behind each sequence is summed too), 'past_max_len_unwritten' (the rows from
    pos_offset + max_len on left as they were), 'offsets32' (the element offset of a row taken modulo 2^32 as a signed 32-bit number,
    for a dX whose row stride were LD32: row t reads row (t mod 16) if that is below 8, nothing otherwise)."""
    assert defect is None or defect in DEFECTS, defect
    T, E = dx.shape
    x32 = dx.float().cpu()
    acc = torch.zeros(P + 1, E, dtype=torch.float32)             # accumulators start at +0.0 (one spare row for 'offset_plus_one')
    off = pos_offset + (1 if defect == 'offset_plus_one' else 0)
    cu = [int(c) for c in cu_lens.tolist()]
    for b in range(len(cu) - 1):                                 # sequences in ascending order
        s, n = cu[b], cu[b + 1] - cu[b]
        if defect == 'len_ge':
            n += 1
        n = min(n, max_len, T - s)                               # (a row outside [0, T) is skipped)
        if defect == 'drop_last' and cu[b + 1] - cu[b] > 0:
            n = min(n, cu[b + 1] - cu[b] - 1)
        if n <= 0:
            continue                                             # a sequence too short for a row enters nothing
        rows = x32[s:s + n]
        if defect == 'offsets32':
            t = torch.arange(s, s + n)
            src = t % 16
            rows = torch.where((src < 8).unsqueeze(1), x32[src.clamp(max=T - 1)], torch.zeros_like(rows))
        acc[off:off + n] += rows
        if defect == 'bf16_acc':
            acc[off:off + n] = acc[off:off + n].to(torch.bfloat16).float()
    out = torch.full((P, E), PREFILL, dtype=torch.bfloat16)
    out[:] = acc[:P].to(torch.bfloat16)                          # every element is written
    if defect == 'past_max_len_unwritten':
        out[pos_offset + max_len:] = PREFILL
    return out
