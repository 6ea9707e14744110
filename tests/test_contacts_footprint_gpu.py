"""The device-pointer entry point of include/esme_hip_contacts.h inside guard-banded arenas (tests/footprint.py): write containment, read
independence (NaN against zero guards), layout invariance (arena views against contiguous tensors) and an uninitialised, exact-size
workspace -- the discipline tests/test_footprint_gpu.py applies to include/esme_hip.h, with a case list of its own.

Coverage (tests/test_contacts_cpu.py fails when a pointer entry point of the header has no case here):

  entry point                      forms covered
  esme_hip_contact_layer           head dims 16 / 32 / 64 / 128, q_prescaled 0 / 1; q / k column views of one (T, 3E) arena; cu_lens, w, map_off and the
                                   exact-size workspace (esme_hip_contact_workspace_bytes) in arenas of their own; the map an output; two layers (init 1
                                   then 0); lengths 0, 0, 1, 2, 3, 18, 66, 67, 130, 195, 0 (empty sequences first and last)
"""
import pytest
import torch

import contact_bounds as CB
import footprint as fp
import test_footprint_gpu as G
from footprint import Case, Operand

pytestmark = pytest.mark.gpu
DEV = G.DEV
LENGTHS = (0, 0, 1, 2, 3, 18, 66, 67, 130, 195, 0)
CASES = []


def add(id, symbols, build):
    CASES.append(G.Spec(id, tuple('esme_hip_' + s for s in symbols.split()), build))


def contact_case(H, d, qp):
    from esme import _hip, _hip_contacts as HC
    layers, cu, scale = CB.make_operands(LENGTHS, H, d, seed=7 + d, qp=bool(qp))
    T, E, B = int(cu[-1]), H * d, len(LENGTHS)
    n, off, total = HC.map_offsets(cu, 1, 1)
    w = torch.randn(2, H, generator=torch.Generator().manual_seed(3))
    nbytes = HC.workspace_bytes(B, T, H)
    ops = [Operand(f'qkv{l}', torch.cat((q, k, torch.zeros(T, E, dtype=G.BF)), 1).contiguous()) for l, (q, k, _) in enumerate(layers)]
    ops += [Operand('cu_lens', cu), Operand('w0', w[0].contiguous()), Operand('w1', w[1].contiguous()), Operand('map_off', off),
            Operand('ws', torch.empty(nbytes, dtype=torch.uint8), 'ws'), G.out('map', (total,), G.F32)]

    def call(v):
        for l in range(2):
            qkv = v[f'qkv{l}']
            G.call_c('esme_hip_contact_layer', G.P(qkv), G.P(qkv) + 2 * E, qkv.stride(0), G.P(v['cu_lens']), B, T, H, d, max(LENGTHS), scale, qp, 1, 1,
                     G.P(v[f'w{l}']), -0.75, int(l == 0), G.P(v['map']), G.P(v['map_off']), G.P(v['ws']), nbytes)
    return Case(f'contact_layer H{H} d{d} qp{qp}', ops, call)


for _H, _d, _qp in [(20, 16, 0), (5, 32, 1), (3, 64, 1), (3, 64, 0), (2, 128, 0)]:
    add(f'contact_layer-H{_H}-d{_d}-qp{_qp}', 'contact_layer contact_workspace_bytes', lambda H=_H, d=_d, qp=_qp: contact_case(H, d, qp))


@pytest.mark.parametrize('spec', CASES, ids=[c.id for c in CASES])
def test_contacts_footprint(spec, monkeypatch):
    from esme import _hip, _hip_contacts
    lib, called = _hip.load(), set()
    _hip_contacts.bind(lib)                  # (typed on the handle itself: the recorder below hands out plain wrappers)

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
