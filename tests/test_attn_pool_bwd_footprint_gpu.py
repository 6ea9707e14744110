"""The device-pointer entry point of include/esme_hip_attn_pool_bwd.h inside guard-banded arenas (tests/footprint.py): write containment,
read independence (NaN against zero guards), layout invariance (arena views against contiguous tensors) and an uninitialised, exact-size
workspace -- the discipline tests/test_footprint_gpu.py applies to include/esme_hip.h, with a case list of its own.

Coverage (tests/test_attn_pool_bwd_cpu.py fails when a pointer entry point of the header has no case here):

  entry point                      forms covered
  esme_hip_attn_pool_bwd           bf16 and fp32 operands; dx present (an output: every row belongs to a sequence and is written) and NULL;
                                   x, d_out and dx in arenas of their own row pitch, U and dU contiguous; cu_lens and the exact-size workspace
                                   (esme_hip_attn_pool_bwd_workspace_bytes) in arenas of their own; lengths 0, 1, 2, 63, 64, 65, 129, 0, 200 and
                                   0, 1, 65, 0, 129, 31, 0 (empty sequences first, inside and last)
"""
import pytest
import torch

import attn_pool_bwd_bounds as PB
import footprint as fp
import test_footprint_gpu as G
from footprint import Case, Operand

pytestmark = pytest.mark.gpu
DEV = G.DEV
CASES = []


def add(id, symbols, build):
    CASES.append(G.Spec(id, tuple('esme_hip_' + s for s in symbols.split()), build))


def bwd_case(lengths, dt, with_dx, C=3):
    from esme import _hip_attn_pool_bwd as HB
    E, H = 64, 4
    J = C * H
    c = PB.make_operands(lengths, E, H, C, dt, seed=17)
    T, B = sum(lengths), len(lengths)
    nbytes = HB.workspace_bytes(B, T, E, H, C)
    assert nbytes == (B + T // 64 + 1) * (2 + 3 * J + 2 * 64 * J + J * E) * 4          # the header's formula
    ops = [Operand('x', c['x']), Operand('cu_lens', c['cu']), Operand('U', c['U'], pad=False), Operand('d_out', c['d_out'].reshape(B, C * E)),
           Operand('ws', torch.empty(nbytes, dtype=torch.uint8), 'ws'), G.out('dU', (J, E), G.F32, pad=False)]
    if with_dx:
        ops.append(G.out('dx', (T, E), dt))

    def call(v):
        dx = v.get('dx')
        G.call_c('esme_hip_attn_pool_bwd', G.P(v['x']), v['x'].stride(0), G.P(v['cu_lens']), B, T, E, H, C, G.P(v['U']), G.P(v['d_out']),
                 v['d_out'].stride(0), G.P(dx), dx.stride(0) if dx is not None else 0, G.P(v['dU']), G.P(v['ws']), nbytes, int(dt == G.F32))
    return Case(f'attn_pool_bwd {dt} dx={with_dx} lengths {lengths}', ops, call)


for _name, _lengths in (('edges', PB.EDGES), ('empties', tuple(G.POOL_LENGTHS))):
    for _dt, _n in ((G.BF, 'bf16'), (G.F32, 'f32')):
        for _dx in (True, False):
            add(f'attn_pool_bwd-{_name}-{_n}-{"dx" if _dx else "nodx"}', 'attn_pool_bwd attn_pool_bwd_workspace_bytes',
                lambda l=_lengths, dt=_dt, dx=_dx: bwd_case(l, dt, dx))


@pytest.mark.parametrize('spec', CASES, ids=[c.id for c in CASES])
def test_attn_pool_bwd_footprint(spec, monkeypatch):
    from esme import _hip, _hip_attn_pool_bwd
    lib, called = _hip.load(), set()
    _hip_attn_pool_bwd.bind(lib)             # (typed on the handle itself: the recorder below hands out plain wrappers)

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
