"""The device-pointer entry point of include/esme_hip_embed_positions_bwd.h inside guard-banded arenas (tests/footprint.py): write
containment, read independence (NaN against zero guards; the guards of cu_lens hold a large out-of-range value) and layout invariance
(arena views against contiguous tensors) -- the discipline tests/test_footprint_gpu.py applies to include/esme_hip.h, with a case list
of its own.

Coverage (tests/test_embed_positions_bwd_cpu.py fails when a pointer entry point of the header has no case here):

  entry point                      forms covered
  esme_hip_embed_positions_bwd     E = 64 and 320 (40 column groups per table row: waves straddle table rows); the length patterns
                                   'empties' (0, 7, 0, 3), 'mixed' (33, 1, 64, 2, 65) and 'b65' (65 sequences of 1 .. 70 rows: nine
                                   rounds of eight sequences, the last ragged) of tests/embed_positions_bwd_bounds.py, with three rows
                                   of d_x behind cu_lens[B]; P = max_len + 2 exactly and max_len + 40; d_x in an arena of its own row
                                   pitch, cu_lens and d_pos (contiguous by the header, every element written: poisoned before the
                                   call) in theirs
"""
import pytest
import torch

import embed_positions_bwd_bounds as PB
import footprint as fp
import test_footprint_gpu as G
from footprint import Case, Operand

pytestmark = pytest.mark.gpu
DEV = G.DEV
CASES = []
PATTERNS = ('empties', 'mixed', 'b65')


def add(id, symbols, build):
    CASES.append(G.Spec(id, tuple('esme_hip_' + s for s in symbols.split()), build))


def embed_positions_bwd_case(case):
    E, cu, T, P, off, max_len = PB.params(case)
    dx, cu_lens, P, off, max_len = PB.make_case(case)
    B = cu_lens.numel() - 1
    ops = [Operand('dx', dx.contiguous()), Operand('cu', cu_lens), G.out('dp', (P, E), pad=False)]

    def call(v):
        G.call_c('esme_hip_embed_positions_bwd', G.P(v['dx']), v['dx'].stride(0), G.P(v['cu']), B, T, E, P, off, max_len, G.P(v['dp']))
    return Case(f'embed_positions_bwd {case[0]}', ops, call)


for _c in PB.GRID:
    if _c[0].split('-')[0] in PATTERNS:
        add(f'embed_positions_bwd-{_c[0]}', 'embed_positions_bwd', lambda c=_c: embed_positions_bwd_case(c))


@pytest.mark.parametrize('spec', CASES, ids=[c.id for c in CASES])
def test_embed_positions_bwd_footprint(spec, monkeypatch):
    from esme import _hip, _hip_embed_positions_bwd
    lib, called = _hip.load(), set()
    _hip_embed_positions_bwd.bind(lib)       # (typed on the handle itself: the recorder below hands out plain wrappers)

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
    case = spec.build()
    res = fp.check(case, DEV)
    monkeypatch.undo()
    assert set(spec.symbols) <= called, f'{spec.id}: labelled {sorted(spec.symbols)}, but the run called {sorted(called)}'
    # the case itself is sound: the output is the emulation's (so every element is finite: a bit-equal NaN would pass the comparisons above)
    c = next(c for c in PB.GRID if spec.id == f'embed_positions_bwd-{c[0]}')
    got = res['nan'].outputs['dp'].view(torch.bfloat16).cpu()
    assert torch.equal(got, PB.emulate(*PB.make_case(c)))
