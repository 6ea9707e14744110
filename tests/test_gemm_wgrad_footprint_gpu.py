"""The device-pointer entry point of include/esme_hip_gemm_wgrad.h inside guard-banded arenas (tests/footprint.py): write containment,
read independence (NaN against zero guards), layout invariance (arena views against contiguous tensors) and an uninitialised, exact-size
workspace -- the discipline tests/test_footprint_gpu.py applies to include/esme_hip.h, with a case list of its own.

Coverage (tests/test_gemm_wgrad_cpu.py fails when a pointer entry point of the header has no case here):

  entry point                      forms covered
  esme_hip_gemm_wgrad              M = 65 (one chunk: the tile kernel writes dW and db itself, no workspace) and M = 4 099 (17 chunks: fp32
                                   partials in the exact-size workspace of esme_hip_gemm_wgrad_workspace_bytes, then the ordered reduce), the
                                   last stage of either ragged; bf16 and fp32 outputs; db present and NULL; (N, K) = (192, 64) and (64, 320):
                                   widths that are 64 mod 128, so half of a 128-column tile lies outside; dy, x and dw in arenas of their
                                   own row pitch, db contiguous
"""
import pytest
import torch

import footprint as fp
import gemm_wgrad_bounds as WB
import test_footprint_gpu as G
from footprint import Case, Operand

pytestmark = pytest.mark.gpu
DEV = G.DEV
CASES = []


def add(id, symbols, build):
    CASES.append(G.Spec(id, tuple('esme_hip_' + s for s in symbols.split()), build))


def wgrad_case(M, N, K, dt, with_db):
    from esme import _hip_gemm_wgrad as HW
    nbytes = HW.workspace_bytes(M, N, K)
    assert nbytes == WB.workspace_bytes(M, N, K) and (nbytes > 0) == (M > 256)       # the header's formula
    ops = [Operand('dy', G.rnd((M, N), 21)), Operand('x', G.rnd((M, K), 22)), G.out('dw', (N, K), dt)]
    if nbytes:
        ops.append(Operand('ws', torch.empty(nbytes, dtype=torch.uint8), 'ws'))
    if with_db:
        ops.append(G.out('db', (N,), dt, pad=False))

    def call(v):
        G.call_c('esme_hip_gemm_wgrad', G.P(v['dy']), v['dy'].stride(0), G.P(v['x']), v['x'].stride(0), M, N, K, G.P(v['dw']), v['dw'].stride(0),
                 G.P(v.get('db')), int(dt == G.F32), G.P(v.get('ws')), nbytes)
    return Case(f'gemm_wgrad M {M} N {N} K {K} {dt} db={with_db}', ops, call)


for _M in (65, 4099):
    for _N, _K in ((192, 64), (64, 320)):
        for _dt, _n in ((G.BF, 'bf16'), (G.F32, 'f32')):
            for _db in (True, False):
                add(f'gemm_wgrad-M{_M}-{_N}x{_K}-{_n}-{"db" if _db else "nodb"}', 'gemm_wgrad gemm_wgrad_workspace_bytes',
                    lambda M=_M, N=_N, K=_K, dt=_dt, db=_db: wgrad_case(M, N, K, dt, db))


@pytest.mark.parametrize('spec', CASES, ids=[c.id for c in CASES])
def test_gemm_wgrad_footprint(spec, monkeypatch):
    from esme import _hip, _hip_gemm_wgrad
    lib, called = _hip.load(), set()
    _hip_gemm_wgrad.bind(lib)                # (typed on the handle itself: the recorder below hands out plain wrappers)

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
