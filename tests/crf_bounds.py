"""float64 restatement, per-element error bound and a CPU emulation for the linear-chain CRF kernels (csrc/crf.hip,
include/esme_hip_crf.h).

`reference` restates the header's definition in float64 by dynamic programming on the operands the kernel is handed: the forward
variables alpha, log Z, the backward variables beta, the marginals d_e = g exp(alpha + beta - log Z), the pairwise marginals summed
into d_transitions, d_start / d_end, and the Viterbi path with the header's tie rule (lowest predecessor, lowest final label).
`brute_force` enumerates every label path of one sequence and validates that restatement (tests/test_crf_cpu.py, at 1e-12).

`bound` follows the kernel's roundings step by step (U32 = 2^-24, E_TRANS = 2^-23 as in tests/error_bounds.py; gamma(n) bounds an fp32
sum of n terms in any order).  One step of the forward recursion for target label j, with w_i the float64 softmax weights of the
predecessors (they sum to 1) and s_i = alpha_prev[i] + A[i][j]:
  [add]   s_i rounded: U32 |s_i|;
  [sub]   s_i - m rounded: U32 |s_i - m|;     [exp] __expf = exp2(x log2 e): the product U32 |x|, v_exp_f32 2 E_TRANS (relative);
  [sum]   gamma(C) relative on the sum of positive terms;
  [log]   __logf = log2(x) ln 2: (2 E_TRANS + U32) |log sum| plus 2 E_TRANS absolute (v_log_f32 near 1 is not relatively accurate);
  [add]   m + log: U32 |lse|;  + e: U32 |alpha|;
so  d_alpha_k[j] = sum_i w_i (d_alpha_{k-1}[i] + U32 |s_i| + 2 U32 |s_i - m| + 2 E_TRANS) + gamma(C) + [log] + U32 (|lse| + |alpha_k[j]|):
the error grows with the chain position and with the magnitude of alpha, and labels that carry no weight carry no error.  The
maximum itself is exact (fmax), and a shift of m cancels.  log Z and the beta recursion have the same form (beta: u = e_next + beta_next
is rounded once more).  The marginals: |d_e| (d_alpha + d_beta + d_logZ + U32 (|alpha + beta| + 2 |alpha + beta - log Z|) + 2 E_TRANS
+ 2 U32); a pairwise term is the product of exp(s_j - m) and g exp(alpha_i + m - log Z): the same with the roundings of both factors.
Sums over rows and sequences: sequence b belongs to part b % P, P = min(B, 1024); a wave adds the rows of its part's sequences in a
running sum (gamma(rows of the sequence + sequences per part) of the absolute terms) and the P partials are added in order (gamma(P)).  Propagated terms carry 1 % for second order; an exponential
below fp32's normal range may be lost whole (TINY per term).
Nothing here is tuned to a GPU run.  `emulate` is a float32 CPU emulation of the stated arithmetic with switches for defects (DEFECTS);
tests/test_crf_cpu.py checks that the bound accepts the faithful emulation and rejects every defect on the cases of
tests/test_crf_gpu.py it applies to.
"""
import itertools
import math

import torch

from error_bounds import E_TRANS, U32

FREE, SKIP = -1, -2
PARTS = 1024                   # ESME_HIP_CRF_PARTS
SECOND_ORDER = 1.01
TINY = 2.0 ** -126            # fp32's smallest normal number: what an exponential below it may lose (flushed or denormal)
NEG = float('-inf')
LENGTHS = (0, 1, 2, 3, 4, 63, 64, 65, 130, 0, 257)       # residues per sequence; + a first and a last SKIP row (the first 0: no row at all)

DEFECTS = ('trans_transposed', 'no_start', 'no_end', 'chain_crosses_sequence', 'skip_row_in_chain', 'constraint_ignored',
           'no_max_subtraction', 'beta_off_by_one', 'grad_unweighted', 'backpointer_wrong_tie')
FLOAT_OUTPUTS = ('logz', 'de', 'dA', 'dstart', 'dend')
OUTPUTS = FLOAT_OUTPUTS + ('path', 'score')


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def _case(name, C, kind='random', tags='mixed'):
    return dict(name=name, C=C, kind=kind, tags=tags)


# every C of {1, 2, 3, 9, 33, 64} with about a fifth of the chain rows free ('mixed') and the rest constrained; all rows free at the
# smallest and largest instantiation; |e| up to 80 ('large'); the nearly forbidden label ('forbidden'); operands on the 2^-4 grid with
# deliberate ties ('grid'), where every fp32 max-plus sum is exact and the path must EQUAL the reference's
CASES = ([_case(f'C{C}-mixed', C) for C in (1, 2, 3, 9, 33, 64)]
         + [_case('C3-free', 3, tags='free'), _case('C64-free', 64, tags='free'), _case('C9-large-free', 9, 'large', 'free'),
            _case('C4-forbidden', 4, 'forbidden'), _case('C2-grid', 2, 'grid'), _case('C9-grid-free', 9, 'grid', 'free'),
            _case('C33-grid', 33, 'grid'), _case('C64-grid', 64, 'grid')])


def rows_of(lengths=LENGTHS):
    """Rows per sequence: the residues and the two frame rows; the first length 0 is a sequence without rows, a later one only a frame."""
    seen0, out = False, []
    for n in lengths:
        out.append(0 if (n == 0 and not seen0) else n + 2)
        seen0 = seen0 or n == 0
    return out


def make_case(case, lengths=LENGTHS):
    """dict: e (T, C), A (C, C), start, end (C) float32; cu (B + 1) int32; tags (T) int32; g (B) float32 (all different)."""
    C, kind = case['C'], case['kind']
    gen = torch.Generator().manual_seed(1000 + 7 * C + len(case['name']))
    rows = rows_of(lengths)
    cu = torch.tensor([0] + list(itertools.accumulate(rows)), dtype=torch.int32)
    T, B = int(cu[-1]), len(rows)
    scale = {'random': 2.0, 'large': 40.0, 'forbidden': 2.0, 'grid': 1.0}[kind]
    e = scale * torch.randn(T, C, generator=gen).clamp(-2, 2)
    A = torch.randn(C, C, generator=gen).clamp(-2, 2)
    start, end = torch.randn(C, generator=gen).clamp(-2, 2), torch.randn(C, generator=gen).clamp(-2, 2)
    if kind == 'grid':                                       # multiples of 2^-4 in [-1, 1]: |path score| <= 260 * 2 + 2 < 2^10
        q = lambda t: (t.clamp(-1, 1) * 16).round() / 16
        e, A, start, end = q(e), q(A), q(start), q(end)
        if C >= 2:                                           # labels 0 and 1 are twins: every step and every final choice ties
            e[:, 1], A[:, 1], A[1, :], start[1], end[1] = e[:, 0], A[:, 0], A[0, :], start[0], end[0]
            A[1, 1] = A[0, 0] = A[0, 1] = A[1, 0]
    if kind == 'forbidden':                                  # label C - 1 only through -10 000 moves; some transitions 100 below the rest
        A[:, C - 1] -= 10000.0
        start[C - 1] -= 10000.0
        A[0, 1] -= 100.0
        A[2, 0] -= 100.0
    tags = torch.full((T,), SKIP, dtype=torch.int32)
    for b in range(B):
        a, z = int(cu[b]), int(cu[b + 1])
        for t in range(a + 1, z - 1):
            r = float(torch.rand((), generator=gen))
            lab = int(torch.randint(0, C - 1 if kind == 'forbidden' else C, (), generator=gen))
            if z - a >= 6 and r < 0.05:
                continue                                     # a SKIP row inside
            tags[t] = FREE if (case['tags'] == 'free' or r < 0.25) else lab
        if kind == 'forbidden' and z - a >= 5:
            tags[a + 2] = C - 1                              # a constrained path through the nearly forbidden label
    tags[tags == SKIP] = torch.tensor([SKIP, -7, C, C + 5, -100], dtype=torch.int32)[torch.arange(int((tags == SKIP).sum())) % 5]
    g = torch.tensor([(0.5 + 0.25 * b) * (-1.0 if b == 3 else 1.0) for b in range(B)], dtype=torch.float32)
    return dict(e=e.float(), A=A.float(), start=start.float(), end=end.float(), cu=cu, tags=tags, g=g)


def chain_rows(cu, tags, C, b, defect=None):
    rows = []
    for t in range(int(cu[b]), int(cu[b + 1])):
        tag = int(tags[t])
        if -1 <= tag < C or defect == 'skip_row_in_chain':
            rows.append((t, tag if (0 <= tag < C and defect != 'constraint_ignored') else FREE))
    return rows


def _lse(s, dim):
    m = s.max(dim=dim, keepdim=True).values
    ms = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    return (ms + torch.log(torch.exp(s - ms).sum(dim=dim, keepdim=True))).squeeze(dim), ms.squeeze(dim)


def _mask(v, tag):
    if tag >= 0:
        keep = torch.zeros_like(v, dtype=torch.bool)
        keep[tag] = True
        v = torch.where(keep, v, torch.full_like(v, NEG))
    return v


def _w(s, dim):
    """softmax weights of s along dim with all -inf -> zeros"""
    w = torch.softmax(s, dim=dim)
    return torch.where(torch.isnan(w), torch.zeros_like(w), w)


def _abs0(x, w):
    """w |x| with 0 * inf = 0"""
    return torch.where(w > 0, w * x.abs(), torch.zeros_like(w))


def reference(e, A, start, end, cu, tags, g, with_bound=False):
    """dict of float64 tensors: logz (B), alpha / beta (T, C; zeros outside chains), de (T, C), dA (C, C), dstart, dend (C), path (T)
    int64 (-100 outside chains), score (B).  with_bound: also 'bound', the dict of per-element bounds of FLOAT_OUTPUTS."""
    e, A, start, end, g = e.double(), A.double(), start.double(), end.double(), g.double()
    T, C = e.shape
    B = cu.numel() - 1
    out = dict(logz=torch.zeros(B, dtype=torch.float64), alpha=torch.zeros(T, C, dtype=torch.float64), de=torch.zeros(T, C, dtype=torch.float64),
               dA=torch.zeros(C, C, dtype=torch.float64), dstart=torch.zeros(C, dtype=torch.float64), dend=torch.zeros(C, dtype=torch.float64),
               path=torch.full((T,), -100, dtype=torch.int64), score=torch.zeros(B, dtype=torch.float64), beta=torch.zeros(T, C, dtype=torch.float64))
    bd = {k: torch.zeros_like(out[k]) for k in FLOAT_OUTPUTS}
    abs_sum = {k: torch.zeros_like(out[k]) for k in ('dA', 'dstart', 'dend')}
    parts = min(B, PARTS)
    per_part = -(-B // parts) if B else 0                     # sequences a part adds up, in ascending order
    log_err = lambda lse, ms: (2 * E_TRANS + U32) * (lse - ms).abs() + 2 * E_TRANS + gamma(C)
    for b in range(B):
        rows = chain_rows(cu, tags, C, b)
        if not rows:
            continue
        n = len(rows)
        al, d_al = [], []
        for k, (t, tag) in enumerate(rows):
            if k == 0:
                v = start + e[t]
                d = U32 * v.abs()
            else:
                s = al[-1].unsqueeze(1) + A                                            # s[i][j]
                lse, ms = _lse(s, 0)
                w = _w(s, 0)
                v = lse + e[t]
                d = ((w * d_al[-1].unsqueeze(1)).sum(0) + U32 * _abs0(s, w).sum(0) + 2 * U32 * _abs0(s - ms.unsqueeze(0), w).sum(0) + 2 * E_TRANS
                     + log_err(lse, ms) + U32 * (lse.abs() + v.abs()))
            v = _mask(v, tag)
            d = torch.where(torch.isinf(v), torch.zeros_like(d), d)
            al.append(v)
            d_al.append(d)
            out['alpha'][t] = v
        f = al[-1] + end
        logz, ms = _lse(f, 0)
        w = _w(f, 0)
        d_logz = ((w * d_al[-1]).sum() + 2 * U32 * _abs0(f, w).sum() + 2 * U32 * _abs0(f - ms, w).sum() + 2 * E_TRANS
                                 + log_err(logz, ms) + U32 * logz.abs())
        out['logz'][b], bd['logz'][b] = logz, d_logz
        be, d_be = [None] * n, [None] * n
        gb = g[b].abs()
        for k in range(n - 1, -1, -1):
            t, tag = rows[k]
            if k == n - 1:
                be[k], d_be[k] = end.clone(), torch.zeros(C, dtype=torch.float64)
            else:
                tn, tagn = rows[k + 1]
                u = _mask(e[tn] + be[k + 1], tagn)
                d_u = torch.where(torch.isinf(u), torch.zeros_like(u), d_be[k + 1] + U32 * u.abs())
                s = A + u.unsqueeze(0)                                                 # s[i][j]
                lse, ms = _lse(s, 1)
                w = _w(s, 1)
                be[k] = lse
                d_be[k] = ((w * d_u.unsqueeze(0)).sum(1) + U32 * _abs0(s, w).sum(1) + 2 * U32 * _abs0(s - ms.unsqueeze(1), w).sum(1)
                                          + 2 * E_TRANS + log_err(lse, ms) + U32 * lse.abs())
                d_be[k] = torch.where(torch.isinf(lse), torch.zeros_like(lse), d_be[k])
                # pairwise marginals of the move rows[k] -> rows[k + 1]
                x = al[k].unsqueeze(1) + s - logz
                xi = torch.exp(x)
                xi = torch.where(torch.isnan(xi), torch.zeros_like(xi), xi)
                fac = al[k] + ms - logz
                fac = torch.where(torch.isinf(al[k]), torch.zeros_like(fac), fac)
                rel = (d_al[k].unsqueeze(1) + d_logz + d_u.unsqueeze(0) + U32 * torch.where(xi > 0, s.abs(), torch.zeros_like(s))
                       + 2 * U32 * torch.where(xi > 0, (s - ms.unsqueeze(1)).abs(), torch.zeros_like(s)) + 2 * E_TRANS
                       + U32 * ((al[k] + ms).abs() + 2 * fac.abs()).unsqueeze(1).nan_to_num(0.0, 0.0, 0.0) + 2 * E_TRANS + 3 * U32)
                out['dA'] += g[b] * xi
                abs_sum['dA'] += gb * xi
                bd['dA'] += gamma(n + per_part) * gb * xi             # the wave's running sum over this sequence's rows and its part's sequences
                bd['dA'] += SECOND_ORDER * gb * xi * rel + 2 * gb * TINY
            x = al[k] + be[k] - logz
            marg = torch.exp(x)
            marg = torch.where(torch.isnan(marg), torch.zeros_like(marg), marg)
            fin = marg > 0
            z = torch.zeros_like(marg)
            rel = (d_al[k] + d_be[k] + d_logz + U32 * torch.where(fin, (al[k] + be[k]).abs(), z) + 2 * U32 * torch.where(fin, x.abs(), z)
                   + 2 * E_TRANS + 2 * U32)
            out['de'][t] = g[b] * marg
            bd['de'][t] = SECOND_ORDER * gb * marg * rel + torch.where(torch.isinf(al[k]), z, gb * TINY + z)
            for name, kk in (('dstart', 0), ('dend', n - 1)):
                if k == kk:
                    out[name] += g[b] * marg
                    abs_sum[name] += gb * marg
                    bd[name] += bd['de'][t]
        for k, (t, _) in enumerate(rows):
            out['beta'][t] = be[k]
        # Viterbi: lowest predecessor on ties (the first maximum), lowest final label
        v, back = None, []
        for k, (t, tag) in enumerate(rows):
            if k == 0:
                best, arg = start.clone(), torch.zeros(C, dtype=torch.int64)
            else:
                s = v.unsqueeze(1) + A
                best = s.max(0).values
                arg = (s == best.unsqueeze(0)).int().argmax(0)                         # the first index that attains the maximum
            back.append(arg)
            v = _mask(best + e[t], tag)
        f = v + end
        y = int((f == f.max()).int().argmax())
        out['score'][b] = f.max()
        for k in range(n - 1, -1, -1):
            out['path'][rows[k][0]] = y
            y = int(back[k][y])
    for k in ('dA', 'dstart', 'dend'):                        # the parts' partials in ascending order (dstart / dend: one term per sequence before)
        bd[k] = bd[k] + gamma(parts + (per_part if k != 'dA' else 0)) * abs_sum[k]
    if with_bound:
        out['bound'] = bd
    return out


def brute_force(e, A, start, end, rows):
    """float64 by enumeration for ONE chain `rows` = [(t, tag)]: (logz, marginals (n, C), pairwise sum (C, C), best path, best score)
    with the tie rule stated as an order on whole paths: among the best paths, the one a backward trace with lowest-index choices finds."""
    e, A, start, end = e.double(), A.double(), start.double(), end.double()
    C, n = e.shape[1], len(rows)
    paths = [p for p in itertools.product(range(C), repeat=n) if all(tag < 0 or p[k] == tag for k, (_, tag) in enumerate(rows))]
    sc = []
    for p in paths:
        s = start[p[0]] + end[p[-1]] + sum(e[rows[k][0], p[k]] for k in range(n)) + sum(A[p[k - 1], p[k]] for k in range(1, n))
        sc.append(s)
    sc = torch.stack(sc)
    logz = torch.logsumexp(sc, 0)
    pr = torch.exp(sc - logz)
    marg, pair = torch.zeros(n, C, dtype=torch.float64), torch.zeros(C, C, dtype=torch.float64)
    for p, q in zip(paths, pr):
        for k in range(n):
            marg[k, p[k]] += q
        for k in range(1, n):
            pair[p[k - 1], p[k]] += q
    best = sc.max()
    # lowest final label, then lowest predecessor at every step going backwards: compare the reversed paths lexicographically
    top = min((tuple(reversed(p)) for p, s in zip(paths, sc) if s == best))
    return logz, marg, pair, list(reversed(top)), best


def worst(got, ref, bnd):
    """max of err / bound (0 / 0 counts as 0; an error over a zero bound, or a non-finite output, counts as inf)"""
    got = got.detach().double().cpu().reshape(-1)
    ref, bnd = ref.double().cpu().reshape(-1), bnd.double().cpu().reshape(-1)
    if not bool(torch.isfinite(got).all()):
        return float('inf')
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd)
    return float(ratio.max()) if ratio.numel() else 0.0


def worst_of(out, ref, exact_path):
    """{name: worst ratio} over the float outputs present in `out`; with `exact_path` (a 'grid' case) also path and score, which must
    EQUAL the reference: 0 or inf."""
    res = {n: worst(out[n], ref[n], ref['bound'][n]) for n in FLOAT_OUTPUTS if out.get(n) is not None}
    if exact_path:
        for n in ('path', 'score'):
            if out.get(n) is not None:
                res[n] = 0.0 if torch.equal(out[n].double().cpu(), ref[n].double()) else float('inf')
    return res


def defect_applies(defect, case):
    """Whether `defect` changes anything the checks of this case look at."""
    C, kind = case['C'], case['kind']
    if defect in ('trans_transposed', 'beta_off_by_one'):
        return C > 1 and not (kind == 'grid' and C == 2)          # (the twins make a 2-label grid case symmetric)
    if defect in ('no_start', 'no_end'):
        return C > 1
    if defect == 'chain_crosses_sequence':
        return True
    if defect == 'skip_row_in_chain':
        return C > 1
    if defect == 'constraint_ignored':
        return C > 1 and case['tags'] == 'mixed'
    if defect == 'no_max_subtraction':
        return kind in ('large', 'forbidden')                     # elsewhere exp neither overflows nor underflows: nothing changes
    if defect == 'grad_unweighted':
        return True
    if defect == 'backpointer_wrong_tie':
        return kind == 'grid' and C > 1
    raise ValueError(defect)


def emulate(e, A, start, end, cu, tags, g, defect=None):
    """float32 emulation of esme_hip_crf_fwd / _bwd / _decode on the CPU: the dict of OUTPUTS.  `defect`: None or one of DEFECTS --
    'trans_transposed' (A read as [j][i]), 'no_start' / 'no_end' (the edge scores dropped), 'chain_crosses_sequence' (the recursion is
    not restarted at a sequence's first chain row), 'skip_row_in_chain' (rows outside the chain taken as free rows),
    'constraint_ignored' (constrained rows taken as free), 'no_max_subtraction' (log sum exp without the shift),
    'beta_off_by_one' (the beta recursion adds the emissions of its own row, not of the next), 'grad_unweighted' (grad_b taken as 1),
    'backpointer_wrong_tie' (the highest predecessor wins a tie)."""
    assert defect is None or defect in DEFECTS, defect
    f32 = torch.float32
    e, A, start, end, g = e.to(f32), A.to(f32), start.to(f32), end.to(f32), g.to(f32)
    if defect == 'trans_transposed':
        A = A.T.contiguous()
    if defect == 'no_start':
        start = torch.zeros_like(start)
    if defect == 'no_end':
        end = torch.zeros_like(end)
    if defect == 'grad_unweighted':
        g = torch.ones_like(g)
    T, C = e.shape
    B = cu.numel() - 1

    def lse(s, dim):
        if defect == 'no_max_subtraction':
            return torch.log(torch.exp(s).sum(dim=dim)), torch.zeros(s.shape[1 - dim], dtype=f32)
        return _lse(s, dim)
    out = dict(logz=torch.zeros(B, dtype=f32), de=torch.zeros(T, C, dtype=f32), dA=torch.zeros(C, C, dtype=f32), dstart=torch.zeros(C, dtype=f32),
               dend=torch.zeros(C, dtype=f32), path=torch.full((T,), -100, dtype=torch.int64), score=torch.zeros(B, dtype=f32))
    carry_a = carry_v = None
    for b in range(B):
        rows = chain_rows(cu, tags, C, b, defect)
        if not rows:
            continue
        n, al, v, back = len(rows), [], None, []
        for k, (t, tag) in enumerate(rows):
            prev_a, prev_v = (al[-1], v) if k else ((carry_a, carry_v) if defect == 'chain_crosses_sequence' else (None, None))
            if prev_a is None:
                a_new, best, arg = start + e[t], start.clone(), torch.zeros(C, dtype=torch.int64)
            else:
                a_new = lse(prev_a.unsqueeze(1) + A, 0)[0] + e[t]
                s = prev_v.unsqueeze(1) + A
                best = s.max(0).values
                hit = (s == best.unsqueeze(0)).int()
                arg = (C - 1 - hit.flip(0).argmax(0)) if defect == 'backpointer_wrong_tie' else hit.argmax(0)
            al.append(_mask(a_new, tag))
            v = _mask(best + e[t], tag)
            back.append(arg)
        carry_a, carry_v = al[-1], v
        logz = lse((al[-1] + end).unsqueeze(1), 0)[0][0]
        out['logz'][b] = logz
        f = v + end
        y = int((f == f.max()).int().argmax())
        out['score'][b] = f.max()
        for k in range(n - 1, -1, -1):
            out['path'][rows[k][0]] = y
            y = int(back[k][y])
        u = None
        for k in range(n - 1, -1, -1):
            t, tag = rows[k]
            if u is None:
                beta = end.clone()
            else:
                s = A + u.unsqueeze(0)
                beta, ms = lse(s, 1)
                fac = g[b] * torch.exp((al[k] + ms) - logz)
                out['dA'] += fac.unsqueeze(1) * torch.exp(s - ms.unsqueeze(1))
            marg = g[b] * torch.exp((al[k] + beta) - logz)
            out['de'][t] = marg
            if k == n - 1:
                out['dend'] += marg
            if k == 0:
                out['dstart'] += marg
            src = e[t] if defect != 'beta_off_by_one' else (e[rows[k - 1][0]] if k else e[t])
            u = _mask(src + beta, tag)
    return out
