"""The device-pointer entry point of include/esme_hip_segment_mean_bwd.h inside guard-banded arenas (tests/footprint.py): write
containment, read independence (NaN against zero guards; the guards of cu_lens hold a large out-of-range value) and layout invariance
(arena views against contiguous tensors) -- the discipline tests/test_footprint_gpu.py applies to include/esme_hip.h, with a case list
of its own.

Coverage (tests/test_segment_mean_bwd_cpu.py fails when a pointer entry point of the header has no case here):

  entry point                      forms covered
  esme_hip_segment_mean_bwd        bfloat16 and float32; E = 8 (one piece per row), 64 and 1288 (161 pieces: rows straddle waves); the
                                   lengths of tests/segment_mean_bwd_bounds.py (empty sequences, 63 / 64 / 65, 129, 200: the last
                                   32-row tile is ragged), three rows before cu_lens[0] and five after cu_lens[B]; d_y and d_x (every
                                   element written: poisoned before the call) in arenas of their own row pitch, cu_lens in its own
"""
import pytest
import torch

import footprint as fp
import segment_mean_bwd_bounds as SB
import test_footprint_gpu as G
from footprint import Case, Operand

pytestmark = pytest.mark.gpu
DEV = G.DEV
CASES = []


def add(id, symbols, build):
    CASES.append(G.Spec(id, tuple('esme_hip_' + s for s in symbols.split()), build))


def segment_mean_bwd_case(case):
    name, dtype, E = case
    dy, cu, T = SB.make_case(case)
    B = dy.shape[0]
    ops = [Operand('dy', dy), Operand('cu', cu), G.out('dx', (T, E), dtype=dtype)]

    def call(v):
        G.call_c('esme_hip_segment_mean_bwd', G.P(v['dy']), v['dy'].stride(0), G.P(v['cu']), B, T, E, G.P(v['dx']), v['dx'].stride(0),
                 1 if dtype == torch.float32 else 0)
    return Case(f'segment_mean_bwd {name}', ops, call)


for _c in SB.CASES:
    add(f'segment_mean_bwd-{_c[0]}', 'segment_mean_bwd', lambda c=_c: segment_mean_bwd_case(c))


@pytest.mark.parametrize('spec', CASES, ids=[c.id for c in CASES])
def test_segment_mean_bwd_footprint(spec, monkeypatch):
    from esme import _hip, _hip_segment_mean_bwd
    lib, called = _hip.load(), set()
    _hip_segment_mean_bwd.bind(lib)          # (typed on the handle itself: the recorder below hands out plain wrappers)

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
    # the case itself is sound: the output is the definition's (so every element is finite: a bit-equal NaN would pass the comparisons above)
    dy, cu, T = SB.make_case(next(c for c in SB.CASES if spec.id.endswith(c[0])))
    got = res['nan'].outputs['dx'].view(dy.dtype)
    assert SB.equal_bits(got, SB.expected(dy, cu, T))
