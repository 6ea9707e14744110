"""The footprint harness (tests/footprint.py) on torch-on-CPU stand-ins: it accepts a correct GEMM-like and a correct attention-like
entry point and rejects each emulated addressing defect, naming the operand and the position.  No GPU needed."""
import os
import re

import pytest
import torch

import footprint as fp

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grown(v, before=0, after=0, right=0):
    """The view `v` extended by rows before / after it and by columns to its right: what a kernel's pointer arithmetic can reach."""
    rows, cols = v.shape
    return torch.as_strided(v, (rows + before + after, cols + right), v.stride(), v.storage_offset() - before * v.stride(0))


# ------------------------------------------------------------------ a GEMM-like entry point: C = A W^T, bf16, fp32 accumulation

M, N, K = 37, 68, 64


def gemm_case(defect=None):
    g = torch.Generator().manual_seed(1)
    A = torch.randn(M, K, generator=g).to(BF)
    W = torch.randn(N, K, generator=g).to(BF)

    def call(v):
        a, w, c = v['A'], v['W'], v['C']
        acc = a.float() @ w.float().T
        if defect == 'load_row_M_times_zero':            # the last row tile loads row M unclamped and weights it with zero
            acc[M - 1] += 0.0 * (_grown(a, after=1)[M].float() @ w.float().T)
        c.copy_(acc.to(BF))
        if defect == 'store_past_last_row':
            _grown(c, after=1)[M, 0] = 1.0
        elif defect == 'vector_store_spills':            # 16-byte stores (8 bf16) over the last column block, N % 8 == 4
            _grown(c, right=4)[:, 64:72] = 2.0
        elif defect == 'store_row_before':
            _grown(c, before=1)[0, 5] = 3.0
        elif defect == 'write_input_pad':
            _grown(a, right=1)[0, K] = 0.5
    return fp.Case(f'gemm-like[{defect}]', [fp.Operand('A', A), fp.Operand('W', W, pad=False),
                                            fp.Operand('C', torch.empty(M, N, dtype=BF), 'out')], call)


def test_correct_gemm_passes():
    res = fp.check(gemm_case())
    a = res['plain'].outputs['C']
    assert a.shape == (M, N) and torch.equal(a, res['nan'].outputs['C'])


@pytest.mark.parametrize('defect,operand,first,last,nbytes', [
    ('store_past_last_row', 'C', (M, 0), (M, 0), 2),
    ('vector_store_spills', 'C', (0, 68), (M - 1, 71), M * 4 * 2),
    ('store_row_before', 'C', (-1, 5), (-1, 5), 2),
    ('write_input_pad', 'A', (0, K), (0, K), 2),
])
def test_stray_writes_are_rejected(defect, operand, first, last, nbytes):
    with pytest.raises(fp.FootprintError) as e:
        fp.check(gemm_case(defect))
    msg = str(e.value)
    assert 'write containment' in msg and f"operand '{operand}'" in msg, msg
    assert f'{nbytes} bytes' in msg and f'first at (row {first[0]}, col {first[1]})' in msg and f'last at (row {last[0]}, col {last[1]})' in msg, msg


def test_unclamped_load_times_zero_needs_the_nan_fill():
    case = gemm_case('load_row_M_times_zero')
    with pytest.raises(fp.FootprintError) as e:
        fp.check(case)
    msg = str(e.value)
    assert 'read independence' in msg and "output 'C'" in msg and f'first at (row {M - 1}, col 0)' in msg and f'last at (row {M - 1}, col {N - 1})' in msg, msg
    # an all-zero guard fill alone would have missed it: no stray write, and the same bits as the contiguous call
    z, p = fp.run(case, 'zero'), fp.run(case, 'plain')
    assert not z.violations and torch.equal(z.outputs['C'], p.outputs['C'])
    assert torch.equal(z.outputs['C'], fp.run(gemm_case(), 'plain').outputs['C'])


# ------------------------------------------------------------------ an attention-like entry point: packed sequences, one head

LENGTHS = [1, 31, 33, 1]
D = 16
TILE = 32


def attn_case(defect=None):
    T = sum(LENGTHS)
    g = torch.Generator().manual_seed(2)
    q, k, v_ = (torch.randn(T, D, generator=g).to(BF) for _ in range(3))
    cu = torch.tensor([0] + list(torch.tensor(LENGTHS).cumsum(0)), dtype=torch.int32)

    def call(v):
        cl = v['cu_lens'].tolist()
        out = v['o']
        for s0, s1 in zip(cl[:-1], cl[1:]):
            qs, ks, vs = v['q'][s0:s1].float(), v['k'][s0:s1].float(), v['v'][s0:s1].float()
            p = torch.softmax(qs @ ks.T * D ** -0.5, -1)
            o = p @ vs
            if defect == 'tail_tile_reads_next_sequence':     # the tail key tile runs to a multiple of TILE: P is zero there, V is loaded
                S = s1 - s0
                over = -(-S // TILE) * TILE - S
                vx = _grown(v['v'], after=TILE)[s1:s1 + over].float()
                o = o + torch.zeros(S, over) @ vx
            out[s0:s1] = o.to(BF)
    return fp.Case(f'attention-like[{defect}]', [fp.Operand('q', q), fp.Operand('k', k), fp.Operand('v', v_), fp.Operand('cu_lens', cu),
                                                 fp.Operand('o', torch.empty(T, D, dtype=BF), 'out')], call)


def test_correct_attention_passes():
    fp.check(attn_case())


def test_tail_key_tile_over_the_next_sequence_needs_the_nan_fill():
    case = attn_case('tail_tile_reads_next_sequence')
    T = sum(LENGTHS)
    with pytest.raises(fp.FootprintError) as e:
        fp.check(case)
    msg = str(e.value)
    # the tail tiles of the 33-row sequence (rows 32 .. 64) and of the last one run past the operand's last row; the others read real rows of
    # their neighbours, times zero
    assert 'read independence' in msg and "output 'o'" in msg and 'first at (row 32, col 0)' in msg and f'last at (row {T - 1}, col {D - 1})' in msg, msg
    z = fp.run(case, 'zero')
    assert not z.violations and torch.equal(z.outputs['o'], fp.run(attn_case(), 'plain').outputs['o'])


# ------------------------------------------------------------------ a workspace carved by one function and sized by another

BLOCK = 64        # floats per block of the stand-in's workspace


def ws_case(defect=None):
    T, E = 130, 16
    nblk = -(-T // BLOCK)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(T, E, generator=g)
    query = (nblk - (1 if defect == 'size_query_one_block_short' else 0)) * BLOCK * 4

    def call(v):
        ws = torch.as_strided(v['ws'].view(torch.float32), (nblk, BLOCK), (BLOCK, 1))     # the carve-up: one block of partials per 64 rows
        for b in range(nblk):
            part = v['x'][b * BLOCK:(b + 1) * BLOCK].sum(0)
            if defect == 'assumes_zeroed_workspace':
                ws[b, :E] += part
            elif defect == 'stale_workspace_times_zero':      # the block's previous contents enter the new value with a zero weight
                ws[b, :E] = part + 0.0 * ws[b, :E]
            else:
                ws[b, :E] = part
        v['out'].copy_(ws[:, :E].sum(0))
    return fp.Case(f'workspace[{defect}]', [fp.Operand('x', x), fp.Operand('ws', torch.empty(query, dtype=torch.uint8), 'ws'),
                                           fp.Operand('out', torch.empty(E), 'out')], call)


def test_correct_workspace_consumer_passes():
    fp.check(ws_case())


def test_workspace_consumer_that_assumes_zeros_is_rejected():
    with pytest.raises(fp.FootprintError) as e:
        fp.check(ws_case('assumes_zeroed_workspace'))
    assert 'read independence' in str(e.value) and "output 'out'" in str(e.value) and 'first at (row 0, col 0)' in str(e.value)


def test_stale_workspace_times_zero_needs_nan_bytes_in_the_workspace():
    """A workspace is uint8 to the harness and floats to the library: its poison must be a NaN at every float width (0xFF bytes), not the
    finite pattern integer operands get -- 0x7F7F7F7F is 3.4e38 as fp32, and 3.4e38 times zero is zero."""
    case = ws_case('stale_workspace_times_zero')
    a = fp.Arena(case.operands[1], 'nan', 'cpu')
    assert bool(torch.isnan(a.view.view(torch.float32)).all()) and bool(torch.isnan(a.view.view(torch.bfloat16)).all()) and bool(torch.isnan(a.view.view(torch.float16)).all())
    assert bool(torch.isnan(a.buf.view(torch.float32)).all())                       # the guards behind it too
    with pytest.raises(fp.FootprintError) as e:
        fp.check(case)
    assert 'read independence' in str(e.value) and "output 'out'" in str(e.value) and 'first at (row 0, col 0)' in str(e.value)
    z = fp.run(case, 'zero')                                                        # zeros alone, or any finite fill, would have missed it
    assert not z.violations and torch.equal(z.outputs['out'], fp.run(ws_case(), 'plain').outputs['out'])
    finite = torch.full((3 * BLOCK,), 3.0e38)
    assert bool((0.0 * finite == 0).all())


def test_vector_guards_are_capped():
    big = fp.Arena(fp.Operand('ws', torch.empty(3 << 20, dtype=torch.uint8), 'ws'), 'nan', 'cpu')
    assert big.g == 1 and big.buf.shape[0] == 3 and big.ld >= (3 << 20) + 2 * fp.PAD_COLS and big.view.data_ptr() % 16 == 0
    small = fp.Arena(fp.Operand('cu_lens', torch.zeros(8, dtype=torch.int32)), 'nan', 'cpu')
    assert small.g == fp.GUARD_ROWS
    mid = fp.Arena(fp.Operand('c1', torch.zeros(5120)), 'nan', 'cpu')
    assert mid.g * mid.ld * 4 <= fp.VECTOR_GUARD_BYTES < (mid.g + 1) * mid.ld * 4


def test_size_query_one_block_short_is_rejected():
    with pytest.raises(fp.FootprintError) as e:
        fp.check(ws_case('size_query_one_block_short'), plain=False)
    msg = str(e.value)
    n = 2 * BLOCK * 4                                   # the workspace the query announced; the third block lies behind it
    assert 'write containment' in msg and "operand 'ws'" in msg and f'first at (row 0, col {n})' in msg and f'last at (row 0, col {n + 16 * 4 - 1})' in msg, msg


def test_zeroed_workspace_is_left_zero_and_outputs_are_poisoned():
    a = fp.Arena(fp.Operand('ws', torch.empty(64, dtype=torch.uint8), 'ws', zeroed=True), 'nan', 'cpu')
    assert not bool(a.view.any()) and int(a.buf[0, 0]) == 0xFF and int(a.buf[a.g, a.lead + 64]) == 0xFF          # zeroed inside, NaN bytes around
    o = fp.Arena(fp.Operand('o', torch.empty(3, 8, dtype=torch.float16), 'out'), 'nan', 'cpu')
    assert bool(torch.isnan(o.view).all()) and o.view.data_ptr() % 16 == 0 and o.view.stride(0) > 8 + fp.PAD_COLS
    assert o.buf.shape[0] == 3 + 2 * fp.GUARD_ROWS and o.lead >= 64 and o.ld - o.lead - 8 >= 64
    i = fp.Arena(fp.Operand('idx', torch.arange(5, dtype=torch.int64)), 'nan', 'cpu')
    assert i.view.tolist() == [0, 1, 2, 3, 4] and int(i.buf[0, 0]) > 2 ** 60
    c = fp.Arena(fp.Operand('codes', torch.zeros(4, 32, dtype=torch.uint8), pad=False), 'nan', 'cpu')        # integer DATA (not a workspace): out of range, finite
    assert int(c.buf[0, 0]) == 0x7F


# ------------------------------------------------------------------ the coverage table cannot fall behind the header

def _pointer_entry_points():
    text = open(os.path.join(ROOT, 'include', 'esme_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    out = []
    for m in re.finditer(r'\b(esme_hip_\w+)\s*\(([^;{}]*?)\)\s*;', text):
        if '*' in m.group(2):
            out.append(m.group(1))
    return out


def test_every_pointer_entry_point_has_a_footprint_case():
    import test_footprint_gpu as G
    names = _pointer_entry_points()
    assert len(names) >= 50 and 'esme_hip_gemm_bf16_opts' in names and 'esme_hip_abi_version' not in names
    covered = set()
    for c in G.CASES:
        covered.update(c.symbols)
    table = G.__doc__
    for n in names:
        assert n in covered, f'{n}: exported by esme_hip.h with a pointer argument, but no footprint case in tests/test_footprint_gpu.py names it'
        assert re.search(rf'\b{n}\b', table), f'{n}: missing from the coverage table in the docstring of tests/test_footprint_gpu.py'
    assert covered <= set(names), covered - set(names)
    ids = [c.id for c in G.CASES]
    assert len(ids) == len(set(ids))
