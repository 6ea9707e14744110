"""The device-pointer entry point of include/esme_hip_attn_bwd.h inside guard-banded arenas (tests/footprint.py): write containment, read
independence (NaN against zero guards), layout invariance (arena views against contiguous tensors) and an uninitialised, exact-size
workspace -- the discipline tests/test_footprint_gpu.py applies to include/esme_hip.h, with a case list of its own.

Coverage (tests/test_attn_bwd_cpu.py fails when a pointer entry point of the header has no case here):

  entry point                      forms covered
  esme_hip_attn_varlen_bwd         head dims 32 / 64; q / k / v column views of one (T, 3E) arena, dq / dk / dv column views of another (an output:
                                   every row belongs to a sequence and is written); o and dO in arenas of their own row pitch; cu_lens and the exact-size
                                   workspace (esme_hip_attn_varlen_bwd_workspace_bytes) in arenas of their own; lengths 0, 1, 2, 63, 64, 65, 129, 0, 200
                                   and 0, 0, 1, 2, 3, 18, 66, 67, 130, 195, 0 (empty sequences first, inside and last)
"""
import pytest
import torch

import attn_bwd_bounds as AB
import footprint as fp
import test_contacts_footprint_gpu as C
import test_footprint_gpu as G
from footprint import Case, Operand

pytestmark = pytest.mark.gpu
DEV = G.DEV
CASES = []


def add(id, symbols, build):
    CASES.append(G.Spec(id, tuple('esme_hip_' + s for s in symbols.split()), build))


def bwd_case(lengths, H, d):
    from esme import _hip_attn_bwd as HB
    ops_ = AB.make_operands(lengths, H, d, seed=11 + d)
    cu, scale = ops_['cu'], ops_['scale']
    T, E, B = int(cu[-1]), H * d, len(lengths)
    nbytes = HB.workspace_bytes(B, T, H)
    ops = [Operand('qkv', ops_['qkv'].contiguous()), Operand('o', G.rnd((T, E), 5)), Operand('do', ops_['do'].contiguous()), Operand('cu_lens', cu),
           Operand('ws', torch.empty(nbytes, dtype=torch.uint8), 'ws'), G.out('dqkv', (T, 3 * E))]

    def call(v):
        qkv, g = v['qkv'], v['dqkv']
        G.call_c('esme_hip_attn_varlen_bwd', G.P(qkv), G.P(qkv) + 2 * E, G.P(qkv) + 4 * E, qkv.stride(0), G.P(v['o']), v['o'].stride(0),
                 G.P(v['do']), v['do'].stride(0), G.P(v['cu_lens']), B, T, H, d, max(lengths), scale,
                 G.P(g), G.P(g) + 2 * E, G.P(g) + 4 * E, g.stride(0), G.P(v['ws']), nbytes)
    return Case(f'attn_varlen_bwd H{H} d{d} lengths {lengths}', ops, call)


for _name, _lengths in (('edges', AB.LENGTHS), ('contacts', C.LENGTHS)):
    for _H, _d in [(5, 32), (3, 64)]:
        add(f'attn_varlen_bwd-{_name}-H{_H}-d{_d}', 'attn_varlen_bwd attn_varlen_bwd_workspace_bytes', lambda l=_lengths, H=_H, d=_d: bwd_case(l, H, d))


@pytest.mark.parametrize('spec', CASES, ids=[c.id for c in CASES])
def test_attn_bwd_footprint(spec, monkeypatch):
    from esme import _hip, _hip_attn_bwd
    lib, called = _hip.load(), set()
    _hip_attn_bwd.bind(lib)                  # (typed on the handle itself: the recorder below hands out plain wrappers)

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
