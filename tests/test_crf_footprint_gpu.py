"""The device-pointer entry points of include/esme_hip_crf.h inside guard-banded arenas (tests/footprint.py): write containment, read
independence (NaN against zero guards), layout invariance (arena views against contiguous tensors) and uninitialised, exact-size
workspaces -- the discipline tests/test_footprint_gpu.py applies to include/esme_hip.h, with a case list of its own.

Coverage (tests/test_crf_cpu.py fails when a pointer entry point of the header has no case here):

  entry point              forms covered
  esme_hip_crf_fwd         six sequences of 0, 3, 12, 0, 70 and 2 rows (empty ones first and inside, more than one batch of rows, two
                           workgroups), framed by SKIP rows, free and constrained rows, C = 9 (the 16-label instantiation, ragged):
                           emissions (a row pitch above C), transitions, start, end, cu_lens, tags (in the NaN run their guards hold
                           a large out-of-range value), logz and alpha (contiguous by the header) each in an arena; and a strided
                           form at C = 33: emissions the second column block of a (T, 2 C + 30) buffer
  esme_hip_crf_bwd         the same two forms, run after the forward on its alpha and logz: grad, d_emissions (an arena of its own
                           pitch), d_transitions, d_start, d_end and the exact-size workspace of esme_hip_crf_bwd_workspace_bytes;
                           without the parameter gradients (and without a workspace) in the strided form
  esme_hip_crf_decode      the same two forms: path (int64; int32 in the strided form), score and the exact-size back-pointer
                           workspace of esme_hip_crf_decode_workspace_bytes
"""
import pytest
import torch

import crf_bounds as CB
import footprint as fp
import test_footprint_gpu as G
from footprint import Case, Operand

pytestmark = pytest.mark.gpu
DEV = G.DEV
CASES = []
LENGTHS = (0, 1, 10, 0, 68, 0)            # residues; rows_of: 0, 3, 12, 2 (a frame only), 70, 2


def add(id, symbols, build):
    CASES.append(G.Spec(id, tuple('esme_hip_' + s for s in symbols.split()), build))


def crf_case(C, strided):
    from esme import _hip_crf as HC
    o = CB.make_case(dict(name=f'fp-{strided}', C=C, kind='random', tags='mixed'), LENGTHS)
    T, B = o['e'].shape[0], o['cu'].numel() - 1
    assert CB.rows_of(LENGTHS) == [0, 3, 12, 2, 70, 2] and T == 89
    nb, nd = HC.bwd_workspace_bytes(B, T, C), HC.decode_workspace_bytes(T, C)
    assert nb == B * (C * C + 2 * C) * 4 and nd == -(-T * C // 16) * 16
    e = Operand('e', o['e'], ld=2 * C + 30, lead=C + 11) if strided else Operand('e', o['e'])      # (a 16-byte aligned base at C = 33)
    ops = [e, Operand('A', o['A'], pad=False), Operand('start', o['start']), Operand('end', o['end']), Operand('cu', o['cu']),
           Operand('tags', o['tags']), Operand('g', o['g']),
           G.out('logz', (B,), G.F32), G.out('alpha', (T, C), G.F32, pad=False), G.out('de', (T, C), G.F32),
           G.out('path', (T,), G.I32 if strided else G.I64), G.out('score', (B,), G.F32),
           Operand('wsd', torch.empty(nd, dtype=torch.uint8), 'ws')]
    if not strided:
        ops += [G.out('dA', (C, C), G.F32, pad=False), G.out('dstart', (C,), G.F32), G.out('dend', (C,), G.F32),
                Operand('wsb', torch.empty(nb, dtype=torch.uint8), 'ws')]

    def call(v):
        common = (G.P(v['e']), v['e'].stride(0), G.P(v['A']), G.P(v['start']), G.P(v['end']), G.P(v['cu']), G.P(v['tags']), B, T, C)
        G.call_c('esme_hip_crf_fwd', *common, G.P(v['logz']), G.P(v['alpha']))
        G.call_c('esme_hip_crf_bwd', *common, G.P(v['alpha']), G.P(v['logz']), G.P(v['g']), G.P(v['de']), v['de'].stride(0), int(not strided),
                 G.P(v.get('dA')), G.P(v.get('dstart')), G.P(v.get('dend')), G.P(v.get('wsb')), 0 if strided else nb)
        G.call_c('esme_hip_crf_decode', *common, G.P(v['path']), int(not strided), -100, G.P(v['score']), G.P(v['wsd']), nd)
    return Case(f'crf C {C} strided {strided}', ops, call)


add('crf-C9-arena', 'crf_fwd crf_bwd crf_decode crf_bwd_workspace_bytes crf_decode_workspace_bytes', lambda: crf_case(9, False))
add('crf-C33-strided', 'crf_fwd crf_bwd crf_decode crf_bwd_workspace_bytes crf_decode_workspace_bytes', lambda: crf_case(33, True))


@pytest.mark.parametrize('spec', CASES, ids=[c.id for c in CASES])
def test_crf_footprint(spec, monkeypatch):
    from esme import _hip, _hip_crf
    lib, called = _hip.load(), set()
    _hip_crf.bind(lib)                       # (typed on the handle itself: the recorder below hands out plain wrappers)

    class Recorder:
        """The loaded library with every esme_hip_* call noted: the case must reach the entry points its coverage label names."""
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if not name.startswith('esme_hip_') or not callable(fn):
                return fn

            def wrapped(*a):
                called.add(name)
                return fn(*a)
            return wrapped
    monkeypatch.setattr(_hip, '_lib', Recorder())
    case = spec.build()                      # (the builder calls the size queries)
    res = fp.check(case, DEV)
    monkeypatch.undo()
    assert set(spec.symbols) <= called, f'{spec.id}: labelled {sorted(spec.symbols)}, but the run called {sorted(called)}'
    # the case itself is sound: every floating-point output holds finite values (bit-equal NaNs would pass the comparisons above)
    for op in case.operands:
        if op.role == 'out' and op.data.dtype.is_floating_point:
            val = res['nan'].outputs[op.name].view(op.data.dtype).float()
            if op.name == 'alpha':                                                    # (-inf by definition at the labels a constrained row excludes)
                val = torch.where(val == float('-inf'), torch.zeros_like(val), val)
            assert bool(torch.isfinite(val).all()), f'{case.name}: output {op.name} is not finite'
    de = res['nan'].outputs['de'].view(torch.float32)
    assert float(de.abs().sum()) > 0                                              # chains exist: the gradients are not trivially zero
    path = res['nan'].outputs['path']
    assert int((path >= 0).sum()) > 60 and int((path == -100).sum()) >= 10
