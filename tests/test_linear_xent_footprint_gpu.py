"""The device-pointer entry points of include/esme_hip_linear_xent.h inside guard-banded arenas (tests/footprint.py): write containment,
read independence (NaN against zero guards), layout invariance (arena views against contiguous tensors) and uninitialised, exact-size
workspaces -- the discipline tests/test_footprint_gpu.py applies to include/esme_hip.h, with a case list of its own.

Coverage (tests/test_linear_xent_cpu.py fails when a pointer entry point of the header has no case here):

  entry point                      forms covered
  esme_hip_linear_xent_fwd         T = 65 (one full tile and one row), E = 320 (two and a half K-chunks), C = 17 (two class blocks, the
                                   second ragged): x, w (a row pitch above E), bias, int64 labels (IGNORE, -7, C and in range; in the NaN
                                   run their guards hold a large out-of-range value), class weights, loss_rows, lse, sums and the
                                   exact-size workspace of esme_hip_linear_xent_fwd_workspace_bytes each in an arena; and a strided form:
                                   x the second column block of a (T, 2 E) buffer, int32 labels, no bias, no class weights, sum
  esme_hip_linear_xent_bwd         the same two forms, run after the forward on its lse and sums: grad, d_x (an arena of its own pitch),
                                   d_w, d_b (contiguous by the header, every element written; float32 in the strided form) and the
                                   exact-size workspace of esme_hip_linear_xent_bwd_workspace_bytes
"""
import pytest
import torch

import footprint as fp
import linear_xent_bounds as LB
import test_footprint_gpu as G
from footprint import Case, Operand

pytestmark = pytest.mark.gpu
DEV = G.DEV
CASES = []


def add(id, symbols, build):
    CASES.append(G.Spec(id, tuple('esme_hip_' + s for s in symbols.split()), build))


def xent_case(T, E, C, strided):
    from esme import _hip_linear_xent as HL
    nf, nb = HL.fwd_workspace_bytes(T), HL.bwd_workspace_bytes(T, E, C)
    assert nf == -(-T // 64) * 8 and nb > 0
    case = dict(name=f'fp-{strided}', T=T, E=E, C=C, bias=not strided, cw=not strided, mean=not strided, i64=not strided, block=None, g=3.0,
                labels='range')
    o = LB.make_case(case)
    x = Operand('x', o['x'], ld=2 * E + 128, lead=E + 64) if strided else Operand('x', o['x'])
    ops = [x, Operand('w', o['w']), Operand('y', o['y']), Operand('g', o['g']),
           G.out('loss_rows', (T,), G.F32), G.out('lse', (T,), G.F32), G.out('sums', (4,), G.F32),
           G.out('dx', (T, E)), G.out('dw', (C, E), G.F32 if strided else G.BF, pad=False),
           Operand('wsf', torch.empty(nf, dtype=torch.uint8), 'ws'), Operand('wsb', torch.empty(nb, dtype=torch.uint8), 'ws')]
    if not strided:
        ops += [Operand('b', o['b']), Operand('cw', o['cw']), G.out('db', (C,), pad=False)]

    def call(v):
        common = (G.P(v['x']), v['x'].stride(0), G.P(v['w']), v['w'].stride(0), G.P(v.get('b')), G.P(v['y']), int(not strided), LB.IGNORE,
                  G.P(v.get('cw')), T, E, C, int(not strided))
        G.call_c('esme_hip_linear_xent_fwd', *common, G.P(v['loss_rows']), G.P(v['lse']), G.P(v['sums']), G.P(v['wsf']), nf)
        G.call_c('esme_hip_linear_xent_bwd', *common, G.P(v['lse']), G.P(v['sums']), G.P(v['g']), 1, G.P(v['dx']), v['dx'].stride(0), 1,
                 G.P(v['dw']), G.P(v.get('db')), int(strided), G.P(v['wsb']), nb)
    return Case(f'linear_xent T {T} E {E} C {C} strided {strided}', ops, call)


for _s in (False, True):
    add(f"linear_xent-T65-E320-C17-{'strided' if _s else 'arena'}",
        'linear_xent_fwd linear_xent_bwd linear_xent_fwd_workspace_bytes linear_xent_bwd_workspace_bytes', lambda s=_s: xent_case(65, 320, 17, s))


@pytest.mark.parametrize('spec', CASES, ids=[c.id for c in CASES])
def test_linear_xent_footprint(spec, monkeypatch):
    from esme import _hip, _hip_linear_xent
    lib, called = _hip.load(), set()
    _hip_linear_xent.bind(lib)               # (typed on the handle itself: the recorder below hands out plain wrappers)

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
            assert bool(torch.isfinite(res['nan'].outputs[op.name].view(op.data.dtype).float()).all()), f'{case.name}: output {op.name} is not finite'
    assert float(res['nan'].outputs['sums'].view(torch.float32)[0, 1]) > 0       # rows were kept: the gradients are not trivially zero
