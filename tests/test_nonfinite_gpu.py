"""NaN and Inf stay inside the sequence, head, row or tensor they occur in, and never come out finite: the kernels under tests/nonfinite.py.

Every case hands a kernel non-finite OPERAND VALUES (footprint.py poisons only what lies around an operand): the rows of one sequence of a
packed batch, the columns of one head, one row of a matrix, one tensor of a list.  Containment: everything outside the unit's output
region is bit-identical to the clean run (a tail tile that reads a neighbour's rows "times zero" fails: 0 * NaN and 0 * Inf are NaN).
Propagation: inside it nothing is finite where the truth is not (nonfinite.LIMITS; the one exception is nonfinite.KNOWN_SWALLOWS, whose
claim the model tests below check: the NaN reaches the logits all the same).

Packed batch of every cu_lens kernel: lengths (65, 33, 1, 0, 130, 64, 7), T = 300: no sequence is longer than the largest row tile (256),
so whatever a tile overhangs lies in a neighbour.  Poisoned sequences, one per run: 1 (partial tiles on both sides), 2 (a single row),
4 (after an empty sequence, before an exact tile).  The head unit is head 1.  Operand builders and configuration tables are those of the
footprint and bound tests, imported (their module-level batches replaced by this one for the duration of a test).

Run with -s: one line per family (cases, units, poisoned runs, KNOWN_SWALLOWS entries used): profiles/nonfinite.txt.
"""
import os
import tempfile

import pytest
import torch

import gemm_operands as gops
import gemm_path as gp
import gemm_persistent_cases as pc
import nonfinite as nf
import optim_bounds as OB
import segment_mean_bwd_bounds as SB
import test_attn_bwd_footprint_gpu as FBWD
import test_attn_maps_footprint_gpu as FMAPS
import test_attn_pool_bwd_footprint_gpu as FPOOLB
import test_contact_features_footprint_gpu as FFEAT
import test_contacts_footprint_gpu as FCONT
import test_footprint_gpu as G
import test_optim_gpu as TO
import test_segment_mean_bwd_footprint_gpu as FSEGB
from nonfinite import Case, Operand, Unit

pytestmark = pytest.mark.gpu
DEV = G.DEV
BF, H16, F32 = G.BF, G.H16, G.F32
LENGTHS = (65, 33, 1, 0, 130, 64, 7)
SEQS = (1, 2, 4)
HEAD = 1
GEOMETRIES = [(16, 8), (32, 8), (64, 4), (128, 2)]
STATS = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    from esme import _hip, _hip_attn_bwd, _hip_attn_maps, _hip_attn_pool_bwd, _hip_contact_features, _hip_contacts, _hip_segment_mean_bwd
    lib = _hip.load()
    for m in (_hip_attn_bwd, _hip_attn_maps, _hip_attn_pool_bwd, _hip_contact_features, _hip_contacts, _hip_segment_mean_bwd):
        m.bind(lib)
    yield
    print('\n[nonfinite] family                      cases   units  poisoned runs  KNOWN_SWALLOWS entries used (cases)')
    for fam, (c, u, p, s) in STATS.items():
        print(f'[nonfinite] {fam:28s}{c:5d}{u:8d}{p:15d}  ' + (', '.join(f'{k} ({n})' for k, n in s.items()) or '-'))
    tot = [sum(v[i] for v in STATS.values()) for i in range(3)]
    used = sorted({k for v in STATS.values() for k in v[3]})
    print(f'[nonfinite] {"total":28s}{tot[0]:5d}{tot[1]:8d}{tot[2]:15d}  {len(used)} of {len(nf.KNOWN_SWALLOWS)} entries: {", ".join(used) or "-"}')
    assert len(used) <= 1, used


def note(family, cases=1, units=0, poisons=0, swallow=None):
    row = STATS.setdefault(family, [0, 0, 0, {}])
    for i, v in enumerate((cases, units, poisons)):
        row[i] += v
    if swallow is not None:
        row[3][swallow] = row[3].get(swallow, 0) + 1


def hold(family, case):
    st = nf.check(case, DEV)
    note(family, 1, st['units'], st['poisons'], case.swallow)
    return st


def cu_of(case):
    return next(op.data for op in case.operands if op.name in ('cu_lens', 'cu')).tolist()


def rows_of(cu, i):
    return slice(cu[i], cu[i + 1])


def cols(start, n):
    return list(range(start, start + n))


def packed_units(cu, parts, outs, d, E, head=True, seqs=SEQS):
    """Sequence units (rows of sequences 1, 2, 4) and the head unit (columns of head 1).  parts: {label: (operand, first column of its
    (T, E) block)}; outs: {output: number of (T, E) column blocks}."""
    units = []
    for i in seqs:
        r = rows_of(cu, i)
        units.append(Unit(f'sequence {i}', {lab: (name, r, cols(c0, E)) for lab, (name, c0) in parts.items()}, {o: (r, None) for o in outs}))
    if head:
        units.append(Unit(f'head {HEAD}', {lab: (name, None, cols(c0 + HEAD * d, d)) for lab, (name, c0) in parts.items()},
                          {o: (None, nf.head_cols(d, HEAD, nb, E)) for o, nb in outs.items()}))
    return units


def single_units(units):
    """One unit per (unit, label), then the unit itself: for kernels whose operands reach different parts of the output."""
    return [Unit(f'{u.name} / {lab}', {lab: v}, u.affects, u.must) for u in units for lab, v in u.poison.items()]


# ------------------------------------------------------------------ attention forward

ATTN = [(f'bf16-d{d}-v{v}-s{s}-q{q}', dict(d=d, H=H, dtype=BF, variant=v, spec=s, qb=q)) for d, H, v, s, q in G.ATTN_BF16]
for _d, _H in GEOMETRIES:
    ATTN += [(f'fwd-d{_d}', dict(d=_d, H=_H, entry='fwd')), (f'exact-d{_d}', dict(d=_d, H=_H, entry='exact')),
             (f'f16-d{_d}', dict(d=_d, H=_H, dtype=H16, scale=1.0)), (f'f16-exact-d{_d}', dict(d=_d, H=_H, dtype=H16, exact=True, scale=1.0))]
    if _d in (32, 64):
        ATTN += [(f'bf16-prescaled-d{_d}', dict(d=_d, H=_H, dtype=BF, variant=0, prescaled=True)),
                 (f'f16-prescaled-d{_d}', dict(d=_d, H=_H, dtype=H16, prescaled=True, scale=1.0))]


@pytest.mark.parametrize('kw', [k for _, k in ATTN], ids=[i for i, _ in ATTN])
def test_attention_forward(kw):
    f = G.attn_case(lengths=list(LENGTHS), **kw)
    d, E = kw['d'], kw['d'] * kw['H']
    outs = {op.name: 1 for op in f.operands if op.role == 'out'}
    parts = {'q': ('qkv', 0), 'k': ('qkv', E), 'v': ('qkv', 2 * E)}
    hold('attention forward', Case.of(f, packed_units(cu_of(f), parts, outs, d, E)))


PAIR = [('split', d, H, None) for d, H in GEOMETRIES] + [('qkpair_opts', d, H, v) for d, H, v in [(16, 8, 0), (16, 8, 1), (32, 8, 0), (32, 8, 1), (32, 8, 2),
                                                                                                  (64, 4, 0), (64, 4, 1), (64, 4, 2)]]


@pytest.mark.parametrize('kind,d,H,variant', PAIR, ids=[f'{k}-d{d}-v{v}' for k, d, H, v in PAIR])
def test_attention_forward_pair_operands(kind, d, H, variant, monkeypatch):
    """attn_varlen_split ([hi (3E) | lo (3E)] in, [hi | lo] out) and attn_varlen_qkpair ([q k hi | v | q k lo] in): hi and lo are poisoned
    separately, then together."""
    monkeypatch.setattr(G, 'LENGTHS', list(LENGTHS))
    f = G.attn_pair_case(kind, d, H, variant)
    E = d * H
    if kind == 'split':
        parts = {f'{n}_{h}': ('qkv', (3 * j + i) * E) for j, h in enumerate(('hi', 'lo')) for i, n in enumerate('qkv')}
        nb = 2
    else:
        parts = {'q_hi': ('qkv', 0), 'k_hi': ('qkv', E), 'v': ('qkv', 2 * E), 'q_lo': ('qkv', 3 * E), 'k_lo': ('qkv', 4 * E)}
        nb = 1
    hold('attention forward', Case.of(f, packed_units(cu_of(f), parts, {'o': nb, 'o_ordered': nb}, d, E)))


# ------------------------------------------------------------------ attention backward, observers

@pytest.mark.parametrize('H,d', [(5, 32), (3, 64)])
def test_attention_backward(H, d):
    """dq, dk, dv of one sequence / head depend on q, k, v, o and dO of that sequence / head only.  dv = P^T dO reads neither v nor o: those
    two must spoil dq and dk."""
    f = FBWD.bwd_case(LENGTHS, H, d)
    E = H * d
    parts = {'q': ('qkv', 0), 'k': ('qkv', E), 'v': ('qkv', 2 * E), 'o': ('o', 0), 'do': ('do', 0)}
    units = packed_units(cu_of(f), parts, {'dqkv': 3}, d, E)
    per = single_units(units)
    for u in per:
        if u.name.endswith(('/ v', '/ o')):
            rows, c = u.affects['dqkv']
            u.must = {'dqkv': (rows, cols(0, 2 * E) if c is None else [x for x in c if x < 2 * E])}
    hold('attention backward', Case.of(f, per + [Unit(u.name + ' / all', u.poison, u.affects, together_only=True) for u in units]))


@pytest.mark.parametrize('d,weighted,bf16', [(32, False, False), (64, False, False), (64, True, True), (32, True, False)])
def test_attention_maps(d, weighted, bf16, monkeypatch):
    """The maps of one sequence depend on its q and k only.  Heads (2, 0) of 3 are selected: head 1 reaches nothing; head 2 reaches the first
    output block of every sequence (heads form), or the one weighted map."""
    monkeypatch.setattr(FMAPS, 'LENGTHS', LENGTHS)
    f = FMAPS.maps_case(d, weighted, bf16)
    E = FMAPS.H * d
    cu = cu_of(f)
    off = next(op.data for op in f.operands if op.name == 'map_off').tolist()
    n_out = 1 if weighted else len(FMAPS.HEADS)
    parts = {'q': ('qkv', 0), 'k': ('qkv', E)}
    units = []
    for i in SEQS:
        S = LENGTHS[i]
        block = cols(off[i] + FMAPS.SLOT0 * S * S, n_out * S * S)
        units.append(Unit(f'sequence {i}', {lab: (name, rows_of(cu, i), cols(c0, E)) for lab, (name, c0) in parts.items()}, {'map': (None, block)}))
    units.append(Unit(f'head {HEAD} (not selected)', {lab: (name, None, cols(c0 + HEAD * d, d)) for lab, (name, c0) in parts.items()}, {}))
    sel = FMAPS.HEADS[0]
    first = [c for i, S in enumerate(LENGTHS) for c in cols(off[i] + FMAPS.SLOT0 * S * S, S * S)]
    units.append(Unit(f'head {sel} (selected first)', {lab: (name, None, cols(c0 + sel * d, d)) for lab, (name, c0) in parts.items()}, {'map': (None, first)}))
    hold('attention maps', Case.of(f, units))


def _contact_blocks(case, lengths):
    off = next(op.data for op in case.operands if op.name == 'map_off').tolist()
    return [cols(off[i], max(n - 2, 0) ** 2) for i, n in enumerate(lengths)]


@pytest.mark.parametrize('H,d,qp', [(20, 16, 0), (5, 32, 1), (3, 64, 0), (2, 128, 0)])
def test_contact_layer(H, d, qp, monkeypatch):
    """The contact logits of one sequence depend on q and k of that sequence, of both layers; every head enters every logit."""
    monkeypatch.setattr(FCONT, 'LENGTHS', LENGTHS)
    f = FCONT.contact_case(H, d, qp)
    E, cu = H * d, cu_of(f)
    blocks = _contact_blocks(f, LENGTHS)
    parts = {f'{n}{l}': (f'qkv{l}', c0) for l in range(2) for n, c0 in (('q', 0), ('k', E))}
    units = [Unit(f'sequence {i}', {lab: (name, rows_of(cu, i), cols(c0, E)) for lab, (name, c0) in parts.items()}, {'map': (None, blocks[i])}) for i in SEQS]
    every = [c for b in blocks for c in b]
    units.append(Unit(f'head {HEAD}', {lab: (name, None, cols(c0 + HEAD * d, d)) for lab, (name, c0) in parts.items()}, {'map': (None, every)}))
    hold('contact_layer', Case.of(f, single_units(units) + units))


@pytest.mark.parametrize('H,d,qp', [(20, 16, 0), (5, 32, 1), (3, 64, 0), (2, 128, 0)])
def test_contact_features(H, d, qp, monkeypatch):
    """Feature column l H + h at a pair of sequence s depends on q and k of layer l, head h, sequence s."""
    monkeypatch.setattr(FFEAT, 'LENGTHS', LENGTHS)
    f = FFEAT.features_case(H, d, qp)
    E, cu = H * d, cu_of(f)
    pairs = next(op.data for op in f.operands if op.name == 'pairs').reshape(-1, 3)
    units = []
    for l in range(2):
        for n, c0 in (('q', 0), ('k', E)):
            for i in SEQS:
                mine = (pairs[:, 0] == i).nonzero().flatten().tolist()
                units.append(Unit(f'sequence {i} / {n}{l}', {f'{n}{l}': (f'qkv{l}', rows_of(cu, i), cols(c0, E))}, {'feat': (mine, cols(l * H, H))}))
            units.append(Unit(f'head {HEAD} / {n}{l}', {f'{n}{l}': (f'qkv{l}', None, cols(c0 + HEAD * d, d))}, {'feat': (None, [l * H + HEAD])}))
    hold('contact_features', Case.of(f, units))


# ------------------------------------------------------------------ pooling

def pool_case(dt, n_cls):
    from esme import _hip
    E, heads = 320, 20
    B, T = len(LENGTHS), sum(LENGTHS)
    nbytes = _hip.attn_pool_workspace_bytes(B, T, E, heads, n_cls)
    ops = [Operand('x', G.rnd((T, E), 1, dtype=dt)), Operand('cu_lens', G.cu_of(LENGTHS)), Operand('U', G.rnd((n_cls * heads, E), 3, 0.3, F32), pad=False),
           Operand('ws', torch.empty(nbytes, dtype=torch.uint8), 'ws'), G.out('out', (B, n_cls * E), dt)]

    def call(v):
        G.call_c('esme_hip_attn_pool', G.P(v['x']), v['x'].stride(0), G.P(v['cu_lens']), B, T, E, heads, n_cls, G.P(v['U']), G.P(v['ws']), nbytes, G.P(v['out']),
                 v['out'].stride(0), int(dt == F32))
    cu = G.cu_of(LENGTHS).tolist()
    # sequence 4 spans three 64-row chunks.  (No head unit: the folded query of every head reads the whole row of x.)
    units = [Unit(f'sequence {i}', {'x': (rows_of(cu, i), None)}, {'out': (i, None)}) for i in SEQS]
    return Case(f'attn_pool {dt} n_cls {n_cls}', ops, call, units)


@pytest.mark.parametrize('n_cls', [1, 3])
@pytest.mark.parametrize('dt', [BF, F32], ids=['bf16', 'f32'])
def test_attn_pool(dt, n_cls):
    hold('attn_pool', pool_case(dt, n_cls))


@pytest.mark.parametrize('n_cls', [1, 3])
@pytest.mark.parametrize('dt', [BF, F32], ids=['bf16', 'f32'])
def test_attn_pool_bwd(dt, n_cls):
    """dx rows of a sequence depend on its x rows and its d_out row; dU sums over all sequences by design."""
    f = FPOOLB.bwd_case(LENGTHS, dt, True, n_cls)
    cu = cu_of(f)
    units = [Unit(f'sequence {i}', {'x': (rows_of(cu, i), None), 'd_out': (i, None)}, {'dx': (rows_of(cu, i), None)}) for i in SEQS]
    hold('attn_pool_bwd', Case.of(f, units, reduced=('dU',)))


@pytest.mark.parametrize('dt', [BF, F32], ids=['bf16', 'f32'])
def test_segment_mean(dt, monkeypatch):
    monkeypatch.setattr(G, 'POOL_LENGTHS', list(LENGTHS))
    f = G.segment_mean_case(dt)
    cu = cu_of(f)
    units = [Unit(f'sequence {i}', {'x': (rows_of(cu, i), None)}, {'out': (i, None)}) for i in SEQS]
    units.append(Unit('column 7', {'x': (None, [7])}, {'out': (None, [7])}, {'out': ([i for i, n in enumerate(LENGTHS) if n], [7])}))
    hold('segment_mean', Case.of(f, units))


@pytest.mark.parametrize('case', SB.CASES[:1] + SB.CASES[-1:], ids=lambda c: c[0])
def test_segment_mean_bwd(case, monkeypatch):
    make = SB.make_case
    monkeypatch.setattr(SB, 'make_case', lambda c: make(c, lengths=LENGTHS))
    f = FSEGB.segment_mean_bwd_case(case)
    cu = cu_of(f)
    units = [Unit(f'sequence {i}', {'dy': (i, None)}, {'dx': (rows_of(cu, i), None)}) for i in SEQS]
    hold('segment_mean_bwd', Case.of(f, units))


@pytest.mark.parametrize('dt', [BF, F32], ids=['bf16', 'f32'])
def test_relu_linear(dt):
    """relu(NaN) is NaN: a NaN row of h gives a NaN row of y, not the bias.  relu(-inf) = 0: a finite row is the limit."""
    f = G.pool_case('relu', dt)
    M = f.operands[0].data.shape[0]
    units = [Unit(f'row {r}', {'h': (r, None)}, {'y': (r, None)}) for r in (0, M // 2, M - 1)]
    units += [Unit('one element', {'h': (5, [9])}, {'y': (5, None)}), Unit('w row 2', {'w': (2, None)}, {'y': (None, [2])}),
              Unit('bias 3', {'bias': (None, [3])}, {'y': (None, [3])})]
    hold('relu_linear', Case.of(f, units, op={'h': 'relu'}, neg_inf=True))


# ------------------------------------------------------------------ row operations: T = 130, E = 320, rows 0, 64 and 129

RT, RE = 130, 320
ROWS = (0, 64, 129)


def row_units(case, ins, outs, rows=ROWS):
    return [Unit(f'row {r}', {n: (r, None) for n in ins}, {n: (r, None) for n in outs}) for r in rows]


def io_names(case):
    ins = [op.name for op in case.operands if op.role in ('in', 'inout') and op.data.dtype.is_floating_point and op.data.dim() == 2 and op.data.shape[0] == op_rows(case)]
    outs = [op.name for op in case.operands if op.role in ('out', 'inout') and op.data.dim() == 2 and op.data.shape[0] == op_rows(case)]
    return ins, outs


def op_rows(case):
    return max(op.data.shape[0] for op in case.operands if op.data.dim() == 2)


@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('kind', ['bf16', 'f32', 'split', 'split_pair', 'split_checked'])
def test_layernorm(kind, bias):
    f = G.ln_case(kind, RT, RE, bias)
    outs = [op.name for op in f.operands if op.role == 'out']
    hold('layernorm', Case.of(f, row_units(f, ['x'], outs), reduced=('flag',)))


@pytest.mark.parametrize('kind', ['residual', 'residual_init', 'operand_bf16', 'operand_f16', 'operand_pair', 'operand_scaled', 'operand_guarded',
                                  'pair_to_f32_bf16', 'pair_to_f32_f16', 'row_sums'])
def test_stream_row_operations(kind):
    """residual_f32, stream_operand (plain, pair, scaled, guarded: col_absmax is a maximum over all rows by design), pair_to_f32, row_sums."""
    f = G.stream_case(kind, RT, RE)
    ins, outs = io_names(f)
    units = row_units(f, ins, outs)
    if kind in ('operand_scaled', 'operand_guarded'):          # [hi | extension tile | lo]: the tile holds the three selected channels, then zeros
        for u in units:
            r = u.affects['x16'][0]
            u.must = dict(u.affects, x16=(r, cols(0, RE) + cols(RE, 3) + cols(RE + 64, RE)))
    hold('stream row operations', Case.of(f, units, reduced=('absmax',)))


@pytest.mark.parametrize('d,H', GEOMETRIES)
@pytest.mark.parametrize('kind', ['bf16', 'f16', 'split', 'split_f16'])
def test_rotary(kind, d, H, monkeypatch):
    monkeypatch.setattr(G, 'ROT_LENGTHS', [1, 63, 65, 1])                           # T = 130: rows 0, 64 (the first of the third sequence) and 129
    f = G.rotary_case(kind, d, H)
    hold('rotary', Case.of(f, row_units(f, ['qkv'], ['qkv'])))


@pytest.mark.parametrize('d,H', [(64, 15), (32, 8)])
@pytest.mark.parametrize('form', ['bf16', 'bf16_scaled', 'f16', 'f16_guarded', 'f16_scaled'])
def test_qk_norm_rotary(form, d, H, monkeypatch):
    """All five forms; qk_sumsq is a maximum over all rows by design.  The LayerNorm runs over all heads of q (of k): the columns of one head
    of q spoil the q block of every row, and nothing of k or v."""
    monkeypatch.setattr(G, 'ROT_LENGTHS', [1, 63, 65, 1])
    f = G.qk_norm_case(form, d, H)
    E = d * H
    units = row_units(f, ['qkv'], ['qkv'])
    units.append(Unit(f'head {HEAD} of q', {'qkv': (None, cols(HEAD * d, d))}, {'qkv': (None, cols(0, E))}))
    units.append(Unit(f'head {HEAD} of k', {'qkv': (None, cols(E + HEAD * d, d))}, {'qkv': (None, cols(E, E))}))
    hold('qk_norm_rotary', Case.of(f, units, reduced=('sumsq',)))


@pytest.mark.parametrize('log', [0, 1])
@pytest.mark.parametrize('V', [33, 64])
@pytest.mark.parametrize('dt', [BF, F32], ids=['bf16', 'f32'])
def test_softmax_rows(dt, V, log):
    """A poisoned row, and one poisoned score of a row: -inf there is a weight of 0 (log-softmax: -inf), which the table accepts; NaN and
    +inf spoil the whole row."""
    f = G.softmax_case(dt, V, log, RT)
    units = row_units(f, ['x'], ['y']) + [Unit('one score', {'x': (3, [V - 1])}, {'y': (3, None)})]
    hold('softmax_rows', Case.of(f, units, op='score', neg_inf=True))


@pytest.mark.parametrize('kind', ['gather', 'scatter'])
def test_gather_scatter_rows(kind):
    """On the footprint case's own shape (50 rows, 23 indices, E = 320), not T = 130: the units follow its index list -- the first and last
    source rows, a row that a random index picks, and the indices outside [0, rows), which must reach nothing."""
    f = G.gather_case(kind)
    idx = next(op.data for op in f.operands if op.name == 'idx').tolist()
    R = 50
    if kind == 'gather':
        units = [Unit(f'source row {r}', {'src': (r, None)}, {'dst': ([j for j, i in enumerate(idx) if i == r], None)}) for r in (0, idx[7], R - 1)]
    else:
        units = [Unit(f'source row {j}', {'src': (j, None)}, {'dst': ([idx[j]] if 0 <= idx[j] < R else [], None)}) for j in (0, 1, 2, 10, len(idx) - 1)]
    hold('gather / scatter rows', Case.of(f, units))


# ------------------------------------------------------------------ GEMM: M = 257, N = 384, K = 128

GM, GN, GK = 257, 384, 128
GEMM_FORMS = ['none', 'nobias', 'gelu', 'residual', 'residual_inplace', 'stats', 'resid32', 'f16_pair_stream', 'swiglu', 'ln_fold', 'ln_fold_dc20',
              'ln_fold_outlier', 'ln_fold_gelu', 'rotary_d64', 'lora_xu']


def gemm_case(form, tile):
    """(footprint case, N): the forms of tests/test_footprint_gpu.py at this shape; the LayerNorm fold also on the 'dc20' and 'outlier'
    operands of tests/gemm_operands.py; the fused rotary at head dim 64 (N = 576: three heads)."""
    N = 576 if form == 'rotary_d64' else GN
    base = {'ln_fold_dc20': 'ln_fold', 'ln_fold_outlier': 'ln_fold', 'rotary_d64': 'rotary'}.get(form, form)
    f = G.gemm_case(base, GM, N, GK, tile, -1)
    if form in ('ln_fold_dc20', 'ln_fold_outlier'):
        x, wp, c1, c2 = (t.cpu() for t in gops.ln_fold_operands(GM, GK, N, 5, form.split('_')[-1], 'cpu'))
        xd = x.double()
        data = {'A': x, 'W': wp, 'c1': c1, 'c2': c2, 'sums': torch.stack((xd.sum(1), (xd * xd).sum(1)), 1).float()}
        for op in f.operands:
            if op.name in data:
                assert data[op.name].shape == op.data.shape and data[op.name].dtype == op.data.dtype, op.name
                op.data = data[op.name].contiguous()
    return f, N


def gemm_units(form, f, N):
    ops = {op.name: op for op in f.operands}
    a_name = 'xu' if form == 'lora_xu' else 'A'
    M = GM

    def out_cols(c):
        """The output columns row c of W (element c of the bias, of c1 / c2) feeds: {output: (may depend, must be non-finite)}."""
        if form == 'swiglu':                               # gate and fc rows interleaved in blocks of 32: both feed column 32 (c / 64) + c % 32
            return {'C': [c // 64 * 32 + c % 32]}
        if form == 'rotary_d64':                           # q and k columns rotate with their partner of the head; v columns stand alone
            E, d = N // 3, 64
            return {'C': [c] if c >= 2 * E else sorted({c, c // d * d + (c % d + d // 2) % d})}
        if form == 'f16_pair_stream':                      # [hi | extension tile | lo]: both halves, and the extension column of a selected channel
            sel = ops['sel'].data.tolist()
            return {'pair': [c, N + 64 + c] + ([N + sel.index(c)] if c in sel else [])}
        return {'C': [c]}

    def row_outs(r):
        o = {}
        if 'C' in ops:
            o['C'] = (r, None)
        if 'stats' in ops:
            o['stats'] = ([r + b * M for b in range(ops['stats'].data.shape[0] // M)], None)
        if 'x32' in ops:
            o['x32'] = (r, None)
        if 'pair' in ops:
            o['pair'] = (r, None)
        return o

    def col_outs(c):
        o = {n: (None, cs) for n, cs in out_cols(c).items()}
        if 'stats' in ops:                                 # one partial per column tile (128 or 256 columns): only the tile that holds the column
            o['stats'] = (stat_rows(c), None)
        if 'x32' in ops:
            o['x32'] = (None, [c])
        return o

    def stat_rows(c):
        nblk = ops['stats'].data.shape[0] // M
        bn = 256 if nblk == -(-N // 256) else 128
        assert nblk == -(-N // bn)
        return cols(c // bn * M, M)

    def col_must(c):
        o = {n: (None, cs[:2] if form == 'f16_pair_stream' else cs) for n, cs in out_cols(c).items()}
        if 'stats' in ops:
            o['stats'] = (stat_rows(c), None)
        if 'x32' in ops:
            o['x32'] = (None, [c])
        return o

    units = []
    for r in (0, 128, 256):
        ins = {a_name: (r, None)}
        for n in ('resid', 'x32', 'pair'):
            if n in ops and ops[n].role in ('in', 'inout'):
                ins[n] = (r, None)
        if form == 'residual_inplace':
            ins['C'] = (r, None)
        must = None
        if 'pair' in ops:                                  # the extension tile holds the selected channels, then zeros
            must = {'pair': (r, cols(0, N) + cols(N, len(ops['sel'].data)) + cols(N + 64, N))}
        units.append(Unit(f'A row {r}', ins, row_outs(r), must))
    last = N - 1
    for c in (0, 127, last):
        units.append(Unit(f'W row {c}', {'W': (c, None)}, col_outs(c), col_must(c)))
    vec = ['c1', 'c2'] if 'c1' in ops else [] if form in ('nobias', 'swiglu') else ['bias']          # (the SwiGLU epilogue adds no bias)
    for n in vec:
        units.append(Unit(f'{n} element 130', {n: (None, [130])}, col_outs(130), col_must(130)))
    if 'sums' in ops:
        units.append(Unit('LayerNorm sums row 128', {'sums': (128, None)}, row_outs(128)))
    return units


@pytest.mark.parametrize('tile', [1, 2])
@pytest.mark.parametrize('form', GEMM_FORMS)
def test_gemm_forms(form, tile):
    """A rows 0, 128, 256 reach the same rows of C, stats_out and the stream; W rows 0, 127 and the last reach their output column (SwiGLU:
    the column they feed; rotary: the column and its partner in the head); one bias (c1, c2) element; one row of the LayerNorm sums.  The
    GELU after the LayerNorm fold is nonfinite.KNOWN_SWALLOWS['gelu_deg5_ln_fold']: containment only."""
    f, N = gemm_case(form, tile)
    op = {'A': 'gelu', 'W': 'gelu', 'bias': 'gelu'} if form == 'gelu' else 'linear'
    hold('gemm forms', Case.of(f, gemm_units(form, f, N), op=op, reduced=('absmax',), swallow='gelu_deg5_ln_fold' if form == 'ln_fold_gelu' else None))


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


@pytest.mark.parametrize('K', pc.SEAM_K)
@pytest.mark.parametrize('form', pc.SEAM_FORMS)
def test_persistent_gemm_seam(form, K):
    """Every A row of the tiles at walk position 0 of three workgroups is poisoned (LayerNorm-fold forms: also their rows of the LayerNorm sums, alone
    and together with A): every tile at walk position >= 1 -- those the same workgroups walk next in particular -- and every other tile is bit-equal
    to the clean run; the poisoned tiles are non-finite."""
    from esme import _hip
    n = torch.cuda.get_device_properties(0).multi_processor_count & ~7
    M, N = pc.shape('two_walks', form, n)
    pc.assert_premise(form, 'two_walks', M, N, n)
    o = pc.operands(form, M, N, K, hip=_hip)
    clean = pc.launch(o, _hip, 1)
    pc.check_written(f'{form} clean', clean)
    tm, tn, gm, gn = gp.raster(M, N, K, 0, 0)
    assert tn == 1
    owner, position = gp.walks(tm * tn, n)
    chosen = (0, n // 2 + 1, n - 1)
    tiles = [gp.tile_coords(pid, tm, tn, gm, gn)[0] for pid in range(tm) if owner[pid] in chosen and position[pid] == 0]
    nxt = [gp.tile_coords(pid, tm, tn, gm, gn)[0] for pid in range(tm) if owner[pid] in chosen and position[pid] == 1]
    assert len(tiles) == 3 and len(nxt) == 3
    rows = torch.zeros(M, dtype=torch.bool)
    for t in tiles:
        rows[t * 256:(t + 1) * 256] = True
    keep = (~rows).to(DEV)
    swallow = form == 'bf16_gelu_ln'
    # a LayerNorm-fold form reads the row statistics, not A, for its per-row strip (mean, rstd): the sums rows of the same tiles are an operand of
    # their own, poisoned alone and together with A -- a strip left over from the previous tile, times zero, then shows in the next tile
    groups = [('a',)] + ([('sums',), ('a', 'sums')] if o['lnf'] else [])
    runs = 0
    for group, kind in [(g, k) for g in groups for k in ('nan', '+inf')]:
        o2 = dict(o)
        if 'a' in group:
            o2['a'] = o['a'].clone()
            _bits(o2['a'])[rows.to(DEV)] = nf.poison_value(kind, o2['a'].dtype).to(DEV)
        if 'sums' in group:
            sums = o['sums'].clone()
            assert sums.shape == (1, M, 2) and o['ln'][0] is o['sums']
            _bits(sums)[0, rows.to(DEV)] = nf.poison_value(kind, sums.dtype).to(DEV)
            o2['sums'], o2['ln'] = sums, (sums,) + tuple(o['ln'][1:])
        got = pc.launch(o2, _hip, 1)
        runs += 1
        what = f'{form} K {K} operand {" + ".join(group)} poison {kind}'
        for name in clean:
            g, c = (_bits(t[name]) for t in (got, clean))
            if name == 'stats':
                g, c = g.transpose(0, 1), c.transpose(0, 1)
            bad = (g[keep] != c[keep]).flatten(1).any(1)
            if bool(bad.any()):
                r = keep.nonzero().flatten()[bad.nonzero().flatten()]
                raise AssertionError(f'{what}: containment: output {name} differs from the clean run in {int(bad.sum())} rows outside the poisoned '
                                     f'tiles {tiles}, first row {int(r[0])} (tile {int(r[0]) // 256}), last row {int(r[-1])} (tile {int(r[-1]) // 256}); the tiles at walk '
                                     f'position 1 of the same workgroups are {nxt}')
            if not swallow:
                vals = got[name].transpose(0, 1) if name == 'stats' else got[name]
                fin = torch.isfinite(vals[~keep].float())
                assert not bool(fin.any()), f'{what}: propagation: output {name} holds {int(fin.sum())} finite values in the poisoned tiles'
    note('gemm persistent seam', 1, 1, runs, 'gelu_deg5_ln_fold' if swallow else None)


# ------------------------------------------------------------------ the guard accumulators of precision 'half'

def test_guard_accumulators_with_a_nan_row(monkeypatch):
    """col_absmax and qk_sumsq are running maxima of bit patterns, read by esme.halfmode.guard_measure.  What a NaN does to them, pinned:
     - col_absmax (stream_operand_guarded, and the fp16 pair-stream residual GEMM): the maximum takes the NaN's bit pattern (above every
       finite one), so the column reads NaN; guard_measure's median of such a site is NaN, `med > 0` is false and the site counts as having
       seen nothing: "in range";
     - qk_sumsq (the LayerNorm-folded q / k projection; qk_norm_rotary_f16_guarded / _f16_scaled of ESM-C): fmaxf drops the NaN, the slot
       keeps the maximum of the other rows: "in range".
    No accumulator reports the NaN -- the range flag does.  The LayerNorm-folded GEMM raises overflow_flag in the same launch, from the row's
    statistics, which are non-finite whenever the row is (they come from the same stream).  The stream kernels, the residual GEMM and
    qk_norm_rotary take no flag: there the NaN is reported by another launch of the same forward, the next LayerNorm-folded GEMM or the final
    LayerNorm (esme_hip_layernorm_split_checked), which read the statistics of that stream:
    test_model_half_guard_reads_in_range_and_the_flag_raises holds ESM-2 and ESM-C to that."""
    from esme import _hip
    for tile in (1, 2):                      # the residual GEMM on the fp16 pair stream: A row 128 (a full pass) and row 256 (the ragged last tile)
        g = nf.Case.of(G.gemm_case('f16_pair_stream', 257, 384, 128, tile, -1), [])
        base = nf.run(g, DEV)['absmax'].view(F32)
        assert bool(torch.isfinite(base).all()) and float(base.min()) > 0
        for r in (128, 256):
            got = nf.run(g, DEV, {'A': ((r, None), 'nan')})['absmax'].view(F32)
            assert bool(torch.isnan(got).all()), f'tile {tile} row {r}: col_absmax of the pair-stream GEMM no longer takes the bit pattern of a NaN'
    monkeypatch.setattr(G, 'ROT_LENGTHS', [1, 63, 65, 1])
    for form in ('f16_guarded', 'f16_scaled'):
        for d, H in [(64, 15), (32, 8)]:
            q = nf.Case.of(G.qk_norm_case(form, d, H), [])
            base, got = (nf.run(q, DEV, p)['sumsq'].view(F32) for p in (None, {'qkv': ((64, None), 'nan')}))
            assert bool(torch.isfinite(got).all()) and bool((got <= base).all()) and float(got.min()) > 0, f'{form} d{d}: qk_sumsq no longer drops a NaN row'
    f = G.stream_case('operand_guarded', RT, RE)
    clean = nf.run(nf.Case.of(f, []), DEV)
    got = nf.run(nf.Case.of(f, []), DEV, {'x32': ((64, None), 'nan')})
    assert bool(torch.isfinite(clean['absmax'].view(F32)).all())
    assert bool(torch.isnan(got['absmax'].view(F32)).all()), 'col_absmax no longer takes the bit pattern of a NaN'
    assert bool(torch.isnan(got['sums'].view(F32)[64]).all()) and torch.equal(got['sums'][:64], clean['sums'][:64])
    # the q / k projection with its guard: A row 128 and its statistics are NaN, as the stream kernels hand them over
    g = G.gemm_case('f16_ln_ext_rotary', 257, 768, 320, 2, -1)
    ops = {op.name: op.data.to(DEV) for op in g.operands}
    M, N, K = 257, 768, 320
    res = {}
    for tag in ('clean', 'nan'):
        stream, sums = ops['stream'].clone(), ops['sums'].clone()
        if tag == 'nan':
            stream[128], sums[128] = float('nan'), float('nan')
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        sumsq = torch.zeros_like(ops['sumsq'])
        C = torch.zeros(M, N, dtype=H16, device=DEV)
        ln = (sums.view(1, M, 2), K - 64, 1e-5, ops['c1'], ops['c2'], flag)
        rot = (ops['cos'], ops['sin'], ops['pos'], ops['cos'].shape[1], 2 * (N // 3))
        with _hip.gemm_options(tile=2, persist=-1):
            _hip.gemm_fused(stream[:, :K], ops['W'], None, out=C, ln=ln, rot=rot, q_scale=0.125 * G.LOG2E, qk_sumsq=sumsq)
        torch.cuda.synchronize()
        res[tag] = (C.cpu(), sumsq.cpu().view(F32), int(flag.item()))
    assert res['clean'][2] == 0 and bool(torch.isfinite(res['clean'][0].float()).all())
    assert res['nan'][2] == 1, 'the launch that drops a NaN row from qk_sumsq must raise the overflow flag'
    assert bool(torch.isnan(res['nan'][0][128].float()).all()) and torch.equal(_bits(res['nan'][0][:128]), _bits(res['clean'][0][:128]))
    assert bool(torch.isfinite(res['nan'][1]).all()) and bool((res['nan'][1] <= res['clean'][1]).all()) and float(res['nan'][1].max()) > 0
    note('guard accumulators', 1, 10, 10)


# ------------------------------------------------------------------ optimizer

def _grad_tensors():
    tensors = OB.make_list('mixed')
    assert sorted({t['numel'] for t in tensors} & {0, 1, 7, 8, 9, OB.CHUNK - 1, OB.CHUNK + 1}) == [0, 1, 7, 8, 9, OB.CHUNK - 1, OB.CHUNK + 1]
    return tensors


def _poisoned(tensors, i, kind):
    out = [dict(t) for t in tensors]
    g = out[i]['grad'].clone()
    g.view(nf._INT_VIEW[g.element_size()])[:] = nf.poison_value(kind, g.dtype)
    out[i]['grad'] = g
    return out


def _outside(pool, span):
    keep = torch.ones(pool.numel(), dtype=torch.bool)
    if span is not None:
        keep[span[0]:span[1]] = False
    return pool.cpu()[keep]


def test_adamw_step_one_poisoned_gradient():
    """The gradient of one tensor of the list is NaN / Inf: parameter, master copy, exp_avg and exp_avg_sq of every other tensor, and every
    byte between the tensors, are bit-equal to the clean step; its own are non-finite."""
    tensors, groups = _grad_tensors(), OB.HPS['a']
    clean = TO.run_step(tensors, groups, 1.0)[0]
    runs = units = 0
    for i, t in enumerate(tensors):
        if t['grad'] is None or t['numel'] == 0:
            continue
        units += 1
        for kind in ('nan', '+inf'):
            pools, _, spans, outs = TO.run_step(_poisoned(tensors, i, kind), groups, 1.0)
            runs += 1
            for k in ('param', 'master', 'm', 'v'):
                assert torch.equal(_outside(pools[k], spans[k][i]), _outside(clean[k], spans[k][i])), \
                    f'tensor {i} (numel {t["numel"]}) poison {kind}: containment: {k} of another tensor differs from the clean step'
                fin = torch.isfinite(outs[i][k].float())
                assert not bool(fin.any()), f'tensor {i} (numel {t["numel"]}) poison {kind}: propagation: {int(fin.sum())} finite values in its own {k}'
    note('adamw_step', 1, units, runs)


def test_grad_accumulate_one_poisoned_gradient():
    from esme import _hip_optim as HO
    tensors = [t for t in _grad_tensors() if t['grad'] is not None]

    def accumulate(ts):
        apool, aviews, aspans = TO.place([dict(t, pdt=OB.F32, gdt=OB.F32, param=torch.zeros(t['numel'])) for t in ts], ('param',))
        acc = [v['param'] for v in aviews]
        for flags in (HO.ACC_INIT, 0):
            pools, views, _ = TO.place(ts, ('grad',))
            table, host, dev = TO._grad_table(ts, views, acc, flags)
            HO.grad_accumulate(host, dev, table.n, 0)
            torch.cuda.synchronize()
        return apool['param'], aspans['param'], acc
    clean = accumulate(tensors)[0]
    runs = units = 0
    for i, t in enumerate(tensors):
        if t['numel'] == 0:
            continue
        units += 1
        for kind in ('nan', '+inf'):
            pool, spans, acc = accumulate(_poisoned(tensors, i, kind))
            runs += 1
            assert torch.equal(_outside(pool, spans[i]), _outside(clean, spans[i])), f'tensor {i} poison {kind}: containment: another accumulator differs'
            assert not bool(torch.isfinite(acc[i]).any()), f'tensor {i} poison {kind}: propagation: finite values in its own accumulator'
    note('grad_accumulate', 1, units, runs)


# ------------------------------------------------------------------ models

MODEL_LENGTHS = (40, 130, 1, 65)
ODD = 25                        # a token id synthetic.random_tokens never draws (4 .. 23, <cls> 0, <eos> 2): every token of sequence 1
_MODELS = {}


def _model(name):
    if name not in _MODELS:
        from esme import ESM, synthetic as syn
        kind, L, E, H, extra = {'esm2': ('esm2', 2, 320, 20, None), 'esmc': ('esmc', 2, 128, 2, None), 'esm1b': ('esm1b', 2, 320, 20, None),
                                'esm2-4bit': ('esm2', 2, 320, 20, '4bit'), 'esm2-lora': ('esm2', 2, 320, 20, 'lora')}[name]
        with tempfile.TemporaryDirectory() as td:
            path = syn.write_checkpoint(os.path.join(td, 'm.safetensors'), f'{kind}_test', L, E, H, seed=23)
            model = ESM.from_pretrained(path, device=DEV, **({'quantization': '4bit'} if extra == '4bit' else {}))
        if extra == 'lora':
            model.add_lora(rank=8, alpha=16, layers=('query', 'key', 'value', 'output', 'ffn_up', 'ffn_down'), adapter_names=['a'])
            g = torch.Generator().manual_seed(2)
            with torch.no_grad():
                for pname, p in model.named_parameters():
                    if '.lora_B.' in pname:                       # (zero after add_lora: give the adapters an effect)
                        p.copy_((torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5).to(p.dtype))
        _MODELS[name] = model
    return _MODELS[name]


def _batch():
    from esme import synthetic as syn
    tokens, cu = syn.random_tokens(list(MODEL_LENGTHS), seed=4), syn.cu_lens_of(list(MODEL_LENGTHS))
    assert ODD not in tokens.tolist()
    tokens[int(cu[1]):int(cu[2])] = ODD
    return tokens.to(DEV), cu.to(DEV), max(MODEL_LENGTHS)


class poisoned_row:
    """Row ODD of the token embedding table set to `value` for the duration of the block."""

    def __init__(self, model, value):
        self.w, self.value = model.embed_tokens.weight, value

    def __enter__(self):
        self.saved = self.w.data[ODD].clone()
        with torch.no_grad():
            self.w[ODD] = self.value                              # (in place: the version counter moves, derived tensors are rebuilt)

    def __exit__(self, *a):
        with torch.no_grad():
            self.w[ODD] = self.saved


def _compare(what, clean, got, skip_cols=()):
    """clean / got: lists of one tensor per sequence.  Sequence 1 non-finite throughout, the others bit-equal to the clean run."""
    assert len(clean) == len(got) == len(MODEL_LENGTHS)
    for i, (c, g) in enumerate(zip(clean, got)):
        c, g = c.cpu(), g.cpu()
        if skip_cols:
            keep = [j for j in range(c.shape[-1]) if j not in skip_cols]
            c, g = c[..., keep], g[..., keep]
        assert bool(torch.isfinite(c.float()).all()), f'{what}: the clean run of sequence {i} is not finite'
        if i == 1:
            fin = torch.isfinite(g.float())
            assert g.numel() > 0 and not bool(fin.any()), f'{what}: propagation: {int(fin.sum())} of {g.numel()} values of the poisoned sequence are finite'
        else:
            assert torch.equal(_bits(c) if c.numel() else c, _bits(g) if g.numel() else g), f'{what}: containment: sequence {i} differs from the clean run'


def _per_sequence(y, cu):
    return [y[a:b] for a, b in zip(cu.tolist()[:-1], cu.tolist()[1:])]


def _tied_columns(model):
    """The logits column of the poisoned token where the LM head shares the embedding table: that column is non-finite for every sequence."""
    w = model.lm_head.final.weight
    return (ODD,) if w.data_ptr() == model.embed_tokens.weight.data_ptr() else ()


MODEL_RUNS = [(n, p, c) for n in ('esm2', 'esmc', 'esm1b') for p in ('fast', 'half', 'exact') for c in (True, False)]
MODEL_RUNS += [('esm2-4bit', 'fast', True), ('esm2-lora', 'fast', True)]          # one 4-bit model; one with all six LoRA adapters


@pytest.mark.parametrize('name,precision,c_forward', MODEL_RUNS, ids=[f'{n}-{p}-c{int(c)}' for n, p, c in MODEL_RUNS])
def test_model_logits(name, precision, c_forward):
    """The embedding row of sequence 1's tokens is NaN, then 3e38 (which overflows in the first LayerNorm): every logit of sequence 1 is
    non-finite -- what common.h promises for the degree-5 GELU site: the NaN reaches the output through the attention branch anyway --
    the logits of the other sequences are bit-equal to the clean run, and in precision 'half' check_overflow() raises."""
    model = _model(name)
    tokens, cu, ml = _batch()
    kw = {'lora_names': ['a']} if name == 'esm2-lora' else {}
    keep = type(model).c_forward
    type(model).c_forward = c_forward
    try:
        if precision == 'half':
            model.set_precision('half', robust=False)
        else:
            model.set_precision(precision)
        with torch.no_grad():
            clean = model(tokens, (cu, ml), **kw)
            model.check_overflow()
            runs = 0
            for value in (float('nan'), 3.0e38):
                with poisoned_row(model, value):
                    got = model(tokens, (cu, ml), **kw)
                    torch.cuda.synchronize()
                    runs += 1
                    if precision == 'half':
                        with pytest.raises(OverflowError):
                            model.check_overflow()
                    _compare(f'{name} {precision} c_forward={c_forward} embedding row {value}', _per_sequence(clean, cu), _per_sequence(got, cu), _tied_columns(model))
            again = model(tokens, (cu, ml), **kw)
            assert torch.equal(again, clean)
            model.check_overflow()
    finally:
        type(model).c_forward = keep
        model.set_precision('fast')
    note('model logits', 1, 1, runs)


@pytest.mark.parametrize('name', ['esm2', 'esmc'])
def test_model_half_guard_reads_in_range_and_the_flag_raises(name):
    """Precision 'half' with its calibrated plan and the plan guard on (ESM-2: the q / k guard of the LayerNorm-folded projection; ESM-C: that of
    qk_norm_rotary): after a forward over a NaN stream the guard's snapshot is finite and says "not stale" (the accumulators do not report a
    NaN: test_guard_accumulators_with_a_nan_row), and the range flag of the same forward raises."""
    from esme import halfmode
    model = _model(name)
    tokens, cu, ml = _batch()
    model.set_precision('half', robust='auto')
    try:
        with torch.no_grad():
            model(tokens, (cu, ml))
            model.check_overflow()
            assert halfmode.guard_snapshot(model) is not None    # (the guard is on; reading it clears the maxima)
            with poisoned_row(model, float('nan')):
                model(tokens, (cu, ml))
                vec = halfmode.guard_snapshot(model)
                assert vec is not None and bool(torch.isfinite(vec).all()) and float(vec[0]) == 0.0, vec[:8]
                with pytest.raises(OverflowError):
                    model.check_overflow()
    finally:
        model.set_precision('fast')
    note('model half guard', 1, 1, 1)


def test_model_heads_and_observers():
    """ClsHead, the attention-pooling head, predict_contacts and attention_maps on the same batch: the poisoned sequence's prediction is
    non-finite (not the last layer's bias), the others are bit-equal."""
    from esme import ContactHead
    from esme.head import ClsHead
    from esme.pooling import LearnedAggregation
    from test_attn_pool_gpu import _randomise
    model = _model('esm2')
    E, H, L = 320, 20, 2
    tokens, cu, ml = _batch()
    cls = _randomise(ClsHead(E, num_cls=3, hidden_dim=512), 42).to(DEV)
    agg = _randomise(LearnedAggregation(4, H, E), 32).to(DEV)
    head = ContactHead(L, H)
    head.regression.weight.data.copy_(torch.randn(1, L * H, generator=torch.Generator().manual_seed(9)))
    model.set_contact_head(head)

    def everything():
        with torch.no_grad():
            rep = model.forward_representation(tokens, (cu, ml))
            out = {'representation': _per_sequence(rep, cu), 'ClsHead': list(cls(rep, cu)), 'ClsHead fp32': list(cls(rep.float(), cu)),
                   'LearnedAggregation': list(agg(rep, (cu, ml))), 'predict_contacts': list(model.predict_contacts(tokens, (cu, ml), logits=True)),
                   'attention_maps': list(model.attention_maps(tokens, (cu, ml))),
                   'attention_maps mean': list(model.attention_maps(tokens, (cu, ml), layers=[-1], heads=[3, 7, 0], head_weights='mean', dtype=BF))}
        torch.cuda.synchronize()
        return {k: [t.clone() for t in v] for k, v in out.items()}
    clean = everything()
    runs = 0
    for value in (float('nan'), 3.0e38):
        with poisoned_row(model, value):
            got = everything()
            runs += 1
        for k in clean:
            _compare(f'{k}, embedding row {value}', clean[k], got[k])
    note('model heads and observers', 1, len(clean), runs)
