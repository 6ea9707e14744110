"""The device-pointer entry point of include/esme_hip_embed_bwd.h inside guard-banded arenas (tests/footprint.py): write containment,
read independence (NaN against zero guards), layout invariance (arena views against contiguous tensors) and an uninitialised, exact-size
workspace -- the discipline tests/test_footprint_gpu.py applies to include/esme_hip.h, with a case list of its own.

Coverage (tests/test_embed_bwd_cpu.py fails when a pointer entry point of the header has no case here):

  entry point                      forms covered
  esme_hip_embed_bwd               T = 255 (one chunk, ragged), 513 (two full chunks and one row) and 2 051 (nine chunks); E = 64 and 320
                                   (a width that is no multiple of a wave's 512 columns: waves straddle chunks); V = 33 and 64 (66 and
                                   128 KiB of LDS); the ids hold the mask id, the pad id, -1 and V, and in the NaN run the guards of the
                                   ids hold a large out-of-range value; d_x in an arena of its own row pitch, tokens, d_table
                                   (contiguous by the header, every element written) and the exact-size workspace of
                                   esme_hip_embed_bwd_workspace_bytes in theirs
"""
import pytest
import torch

import embed_bwd_bounds as EB
import footprint as fp
import test_footprint_gpu as G
from footprint import Case, Operand

pytestmark = pytest.mark.gpu
DEV = G.DEV
CASES = []


def add(id, symbols, build):
    CASES.append(G.Spec(id, tuple('esme_hip_' + s for s in symbols.split()), build))


def embed_bwd_case(T, E, V):
    from esme import _hip_embed_bwd as HE
    nbytes = HE.workspace_bytes(T, E, V)
    assert nbytes == -(-T // EB.ROWS) * V * E * 4 and nbytes > 0           # the header's formula
    tok = EB.make_tokens(T, V, 'skew', 40 + T + V, V - 1, 1)
    ops = [Operand('dx', G.rnd((T, E), 31)), Operand('tok', tok), G.out('de', (V, E), pad=False),
           Operand('ws', torch.empty(nbytes, dtype=torch.uint8), 'ws')]

    def call(v):
        G.call_c('esme_hip_embed_bwd', G.P(v['dx']), v['dx'].stride(0), G.P(v['tok']), T, E, V, V - 1, 1, G.P(v['de']), G.P(v['ws']), nbytes)
    return Case(f'embed_bwd T {T} E {E} V {V}', ops, call)


for _T in (255, 513, 2051):
    for _E in (64, 320):
        for _V in (33, 64):
            add(f'embed_bwd-T{_T}-E{_E}-V{_V}', 'embed_bwd embed_bwd_workspace_bytes', lambda T=_T, E=_E, V=_V: embed_bwd_case(T, E, V))


@pytest.mark.parametrize('spec', CASES, ids=[c.id for c in CASES])
def test_embed_bwd_footprint(spec, monkeypatch):
    from esme import _hip, _hip_embed_bwd
    lib, called = _hip.load(), set()
    _hip_embed_bwd.bind(lib)                 # (typed on the handle itself: the recorder below hands out plain wrappers)

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
    case = spec.build()                      # (the builder calls the size query)
    res = fp.check(case, DEV)
    monkeypatch.undo()
    assert set(spec.symbols) <= called, f'{spec.id}: labelled {sorted(spec.symbols)}, but the run called {sorted(called)}'
    # the case itself is sound: every floating-point output holds finite values (bit-equal NaNs would pass the comparisons above)
    for op in case.operands:
        if op.role == 'out' and op.data.dtype.is_floating_point:
            assert bool(torch.isfinite(res['nan'].outputs[op.name].view(op.data.dtype).float()).all()), f'{case.name}: output {op.name} is not finite'
