"""The non-finite harness (tests/nonfinite.py) on torch-on-CPU stand-ins: it accepts the correct entry points and rejects each emulated
defect with the right check named.  Every containment defect here weights a neighbour's values with ZERO, so with finite data it is
invisible: outputs are bit-equal to the correct ones, a sequence alone equals its slice of the packed batch, and footprint.check passes
(no byte outside an operand is touched).  No GPU needed."""
import pytest
import torch

import footprint as fp
import nonfinite as nf
from nonfinite import Case, Operand, Unit

BF, F32 = torch.bfloat16, torch.float32


def out(name, shape, dtype=F32):
    return Operand(name, torch.empty(shape, dtype=dtype), 'out')


def rejected(case, check, *words):
    with pytest.raises(nf.NonFiniteError) as e:
        nf.check(case)
    msg = str(e.value)
    assert f': {check}: ' in msg, msg
    for w in words:
        assert w in msg, msg
    return msg


# ------------------------------------------------------------------ packed attention, H heads, key tiles of TILE rows

LENGTHS = [5, 33, 1, 0, 40, 32, 7]
D, H, TILE = 8, 3, 32


def cu_of(lengths):
    return torch.tensor([0] + list(torch.tensor(lengths).cumsum(0)), dtype=torch.int32)


def attn_case(defect=None, lengths=LENGTHS):
    T, E = sum(lengths), H * D
    g = torch.Generator().manual_seed(2)
    q, k, v_ = (torch.randn(T, E, generator=g).to(BF) for _ in range(3))

    def call(v):
        cl = v['cu_lens'].tolist()
        n = v['v'].shape[0]
        for s0, s1 in zip(cl[:-1], cl[1:]):
            S = s1 - s0
            if S == 0:
                continue
            for h in range(H):
                c = slice(h * D, (h + 1) * D)
                p = torch.softmax(v['q'][s0:s1, c].float() @ v['k'][s0:s1, c].float().T * D ** -0.5, -1)
                o = p @ v['v'][s0:s1, c].float()
                if defect == 'tail_clamped_to_operand_end':          # the tail key tile runs to a multiple of TILE, clamped to row T - 1, not S - 1: P is zero there
                    over = -(-S // TILE) * TILE - S
                    idx = torch.arange(s1, s1 + over).clamp(max=n - 1)
                    o = o + (torch.zeros(S, over, 1) * v['v'][idx][:, c].float()[None]).sum(1)
                elif defect == 'neighbour_head' and h + 1 < H:       # the V fragment of head h + 1 enters head h with weight 0
                    o = o + 0.0 * (p @ v['v'][s0:s1, (h + 1) * D:(h + 2) * D].float())
                v['o'][s0:s1, c] = o.to(BF)
    ops = [Operand('q', q), Operand('k', k), Operand('v', v_), Operand('cu_lens', cu_of(lengths)), out('o', (T, E), BF)]
    units = [Unit(f'sequence {i}', {n: (nf.seq_rows(lengths, i), None) for n in 'qkv'}, {'o': (nf.seq_rows(lengths, i), None)}) for i in (1, 2, 4) if i < len(lengths)]
    if len(lengths) > 1:
        units.append(Unit('head 1', {n: (None, nf.head_cols(D, 1)) for n in 'qkv'}, {'o': (None, nf.head_cols(D, 1))}))
    return Case(f'attention-like[{defect}]', ops, call, units)


def as_footprint(case):
    return fp.Case(case.name, case.operands, case.call)


def test_correct_attention_passes():
    st = nf.check(attn_case())
    assert st == {'units': 4, 'poisons': 4 * 4 * 2, 'swallows': 0}          # q, k, v alone and together; NaN and +Inf


def test_tail_clamped_to_operand_end_is_rejected_and_invisible_to_finite_checks():
    case = attn_case('tail_clamped_to_operand_end')
    # sequence 1 (rows 5 .. 37) is poisoned: the tail tile of sequence 0 (5 rows, 27 rows of overhang) reads it, times zero
    rejected(case, 'containment', "unit 'sequence 1'", 'operand v', 'poison nan', "output 'o'", 'first at (row 0, col 0)', f'last at (row 4, col {H * D - 1})')
    # with finite data the stand-in IS the correct kernel, by every check the suite had: same bits as the correct one, a sequence alone bit-equal
    # to its slice of the packed batch, and the footprint harness passes (the clamp keeps every read inside the operand)
    packed = nf.run(case)['o']
    assert torch.equal(packed, nf.run(attn_case())['o'])
    for i, n in enumerate(LENGTHS):
        if n == 0:
            continue
        rows = nf.seq_rows(LENGTHS, i)
        alone = attn_case('tail_clamped_to_operand_end', [n])
        for op in alone.operands[:3]:
            op.data = case.operands[alone.operands.index(op)].data[rows].clone()
        assert torch.equal(nf.run(alone)['o'], packed[rows]), i
    fp.check(as_footprint(case))


def test_neighbour_head_is_rejected():
    case = attn_case('neighbour_head')
    rejected(case, 'containment', "unit 'head 1'", 'operand v', 'poison nan', 'first at (row 0, col 0)', f'last at (row {sum(LENGTHS) - 1}, col {D - 1})')
    assert torch.equal(nf.run(case)['o'], nf.run(attn_case())['o'])
    fp.check(as_footprint(case))


# ------------------------------------------------------------------ pooling: partial softmax sums per chunk of CHUNK rows, then a merge

CHUNK = 16
POOL_LENGTHS = [20, 33, 1, 0, 50, 16, 7]


def pool_case(defect=None):
    T, E = sum(POOL_LENGTHS), 8
    g = torch.Generator().manual_seed(3)
    x, u = torch.randn(T, E, generator=g), torch.randn(E, generator=g)

    def call(v):
        cl = v['cu_lens'].tolist()
        slots = []                                                   # (sequence, m, l, o): one per chunk, in packed order
        for s, (s0, s1) in enumerate(zip(cl[:-1], cl[1:])):
            for c0 in range(s0, s1, CHUNK):
                xs = v['x'][c0:min(c0 + CHUNK, s1)]
                sc = xs @ v['u']
                m = sc.max()
                w = torch.exp2(sc - m)
                slots.append((s, m, w.sum(), w @ xs))
        for s in range(len(cl) - 1):
            mine = [i for i, t in enumerate(slots) if t[0] == s]
            if not mine:
                v['out'][s] = 0
                continue
            m = torch.stack([slots[i][1] for i in mine]).max()
            ls = [torch.exp2(slots[i][1] - m) * slots[i][2] for i in mine]
            os_ = [torch.exp2(slots[i][1] - m) * slots[i][3] for i in mine]
            if defect == 'combine_reads_next_slot' and mine[-1] + 1 < len(slots):      # one slot too many, with weight exp2(-inf) = 0
                nxt = slots[mine[-1] + 1]
                a = torch.exp2(torch.tensor(float('-inf')))
                ls.append(a * nxt[2])
                os_.append(a * nxt[3])
            v['out'][s] = sum(os_) / sum(ls)
    ops = [Operand('x', x), Operand('u', u), Operand('cu_lens', cu_of(POOL_LENGTHS)), out('out', (len(POOL_LENGTHS), E))]
    units = [Unit(f'sequence {i}', {'x': (nf.seq_rows(POOL_LENGTHS, i), None)}, {'out': (i, None)}) for i in (1, 2, 4)]
    return Case(f'pool-like[{defect}]', ops, call, units)


def test_correct_pooling_passes():
    nf.check(pool_case())


def test_combine_reads_next_slot_is_rejected():
    case = pool_case('combine_reads_next_slot')
    rejected(case, 'containment', "unit 'sequence 1'", 'operand x', 'poison nan', "output 'out'", 'first at (row 0, col 0)', 'last at (row 0, col 7)')
    assert torch.equal(nf.run(case)['out'], nf.run(pool_case())['out'])
    fp.check(as_footprint(case))


# ------------------------------------------------------------------ a persistent GEMM with a LayerNorm fold: NCU workgroups walk the row tiles

NCU, TM = 3, 8


def seam_case(defect=None):
    M, N, K = 2 * NCU * TM - 3, 12, 16                               # two walks, the last tile ragged
    g = torch.Generator().manual_seed(4)
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)

    def call(v):
        tiles = [(r0, min(r0 + TM, M)) for r0 in range(0, M, TM)]
        for wg in range(NCU):
            strip = None
            for r0, r1 in tiles[wg::NCU]:
                a = v['A'][r0:r1]
                mean, rstd = a.mean(1, keepdim=True), (a.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
                c = rstd * (a @ v['W'].T - mean * v['W'].sum(1))
                if defect == 'stale_strip_over_seam' and strip is not None:      # the previous tile's strip is still in registers: times 0
                    c = c + 0.0 * strip[:r1 - r0]
                strip = rstd
                v['C'][r0:r1] = c
    ops = [Operand('A', A), Operand('W', W, pad=False), out('C', (M, N))]
    first = [r for wg in range(NCU) for r in range(wg * TM, (wg + 1) * TM)]          # the tiles at walk position 0
    units = [Unit('walk position 0', {'A': (first, None)}, {'C': (first, None)}), Unit('row 0', {'A': (0, None)}, {'C': (0, None)}),
             Unit('W row 5', {'W': (5, None)}, {'C': (None, 5)})]
    return Case(f'persistent-gemm-like[{defect}]', ops, call, units)


def test_correct_persistent_gemm_passes():
    nf.check(seam_case())


def test_stale_strip_over_seam_is_rejected():
    case = seam_case('stale_strip_over_seam')
    rejected(case, 'containment', "unit 'walk position 0'", 'operand A', 'poison nan', "output 'C'", f'first at (row {NCU * TM}, col 0)', 'last at (row 44, col 11)')
    assert torch.equal(nf.run(case)['C'], nf.run(seam_case())['C'])
    fp.check(as_footprint(case))


# ------------------------------------------------------------------ y = relu(h) W^T + b

def relu_case(defect=None):
    M, N, K = 9, 5, 16
    g = torch.Generator().manual_seed(5)
    h, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)

    def call(v):
        r = torch.fmax(v['h'], torch.zeros(())) if defect == 'relu_by_max' else torch.relu(v['h'])
        v['y'].copy_(r @ v['w'].T + v['b'])
    ops = [Operand('h', h), Operand('w', w), Operand('b', b), out('y', (M, N))]
    units = [Unit(f'row {r}', {'h': (r, None)}, {'y': (r, None)}) for r in (0, 4, M - 1)]
    return Case(f'relu-linear-like[{defect}]', ops, call, units, op={'h': 'relu'}, neg_inf=True)


def test_correct_relu_passes_and_minus_inf_has_a_limit():
    st = nf.check(relu_case())
    assert st['poisons'] == 3 * 3
    y = nf.run(relu_case(), poison={'h': ((4, None), '-inf')})['y'].view(F32)
    assert bool(torch.isfinite(y).all())                             # relu(-inf) = 0: the table accepts it


def test_relu_by_max_passes_containment_and_is_rejected_by_propagation():
    case = relu_case('relu_by_max')
    msg = rejected(case, 'propagation', "unit 'row 0'", 'operand h', 'poison nan', "output 'y'", 'first at (row 0, col 0)', 'last at (row 0, col 4)')
    assert 'containment' not in msg
    clean, got = nf.run(case)['y'], nf.run(case, poison={'h': ((0, None), 'nan')})['y']
    assert torch.equal(clean[1:], got[1:]) and bool(torch.isfinite(got.view(F32)).all())          # a finite prediction from a NaN row: the bias term survives


def test_a_finite_value_where_the_limit_is_infinite_is_rejected():
    case = relu_case()
    case.call = lambda v: v['y'].copy_(torch.relu(v['h'].clamp(max=1.0e30)) @ v['w'].T + v['b'])      # saturates +Inf (torch.clamp hands NaN on)
    rejected(case, 'propagation', 'poison +inf', "output 'y'")


def test_clean_run_must_be_finite():
    case = relu_case()
    case.operands[2].data[1] = float('inf')
    rejected(case, 'clean run', "output 'y'", 'first at (row 0, col 1)')


# ------------------------------------------------------------------ a multi-tensor optimizer step over chunks of a flat list

OPT_CHUNK = 8
NUMELS = [0, 1, 7, 8, 9, OPT_CHUNK - 1, OPT_CHUNK + 1]


def optim_case(defect=None):
    g = torch.Generator().manual_seed(6)
    ops = []
    for i, n in enumerate(NUMELS):
        ops += [Operand(f'p{i}', torch.randn(n, generator=g), 'inout'), Operand(f'g{i}', torch.randn(n, generator=g)), Operand(f'm{i}', torch.randn(n, generator=g), 'inout')]

    def call(v):
        flat_g = torch.cat([v[f'g{i}'] for i in range(len(NUMELS))])
        start = 0
        for i, n in enumerate(NUMELS):
            gi = v[f'g{i}']
            if defect == 'chunk_straddles_tensors' and n:            # the chunk's statistic spans whatever tensors share the chunk: times 0
                c0, c1 = start // OPT_CHUNK * OPT_CHUNK, -(-(start + n) // OPT_CHUNK) * OPT_CHUNK
                gi = gi + 0.0 * flat_g[c0:c1].sum()
            v[f'm{i}'].mul_(0.9).add_(gi, alpha=0.1)
            v[f'p{i}'].sub_(v[f'm{i}'], alpha=0.01)
            start += n
    units = [Unit(f'tensor {i}', {f'g{i}': (None, None)}, {f'p{i}': (None, None), f'm{i}': (None, None)}) for i, n in enumerate(NUMELS) if n]
    return Case(f'optimizer-like[{defect}]', ops, call, units)


def test_correct_optimizer_passes():
    assert nf.check(optim_case())['units'] == len(NUMELS) - 1


def test_chunk_straddles_tensors_is_rejected():
    case = optim_case('chunk_straddles_tensors')
    rejected(case, 'containment', "unit 'tensor 1'", 'operand g1', 'poison nan', "output 'p2'")
    assert all(torch.equal(a, b) for a, b in zip(nf.run(case).values(), nf.run(optim_case()).values()))


# ------------------------------------------------------------------ the harness itself

def test_poisons_are_what_they_say():
    for dt in (BF, torch.float16, F32, torch.float64):
        idt = nf._INT_VIEW[torch.empty(0, dtype=dt).element_size()]
        assert bool(torch.isnan(nf.poison_value('nan', dt).view(dt))) and int(nf.poison_value('nan', dt)) == int(torch.tensor(fp._poison(Operand('x', torch.empty(1, dtype=dt)), 'nan'), dtype=idt))
        assert float(nf.poison_value('+inf', dt).view(dt)) == float('inf') and float(nf.poison_value('-inf', dt).view(dt)) == float('-inf')


def test_known_swallows_has_one_entry_and_quotes_the_kernel():
    import os
    assert list(nf.KNOWN_SWALLOWS) == ['gelu_deg5_ln_fold']
    where, quote = nf.KNOWN_SWALLOWS['gelu_deg5_ln_fold']
    path, lines = where.split(':')
    a, b = (int(x) for x in lines.split('-'))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = ' '.join(line.strip().lstrip('/ ') for line in open(os.path.join(root, path)).read().splitlines()[a - 1:b])
    for part in quote.split(' [...] '):
        assert part in text, part


def test_a_swallow_skips_propagation_only():
    case = relu_case('relu_by_max')
    case.swallow = 'gelu_deg5_ln_fold'
    assert nf.check(case)['swallows'] == 1
    bad = pool_case('combine_reads_next_slot')
    bad.swallow = 'gelu_deg5_ln_fold'
    rejected(bad, 'containment')


def test_reduced_outputs_get_no_containment_check():
    case = pool_case('combine_reads_next_slot')
    case.reduced = ('out',)
    nf.check(case)
