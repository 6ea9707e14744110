"""The device-pointer entry points of include/esme_hip_dequant_t.h inside guard-banded arenas (tests/footprint.py): write containment, read
independence (NaN / out-of-range guards against zero guards) and, where a contiguous `out` is a legal operand (N a multiple of 8),
layout invariance -- the discipline tests/test_footprint_gpu.py applies to include/esme_hip.h, with a case list of its own.

codes and absmax / scale are contiguous operands (guard rows only); `out` (K, N) sits between pad columns with a row pitch larger than
N, and every element of it must be written (it is poisoned before the call), nothing around it.

Coverage (tests/test_qlora_cpu.py fails when a pointer entry point of the header has no case here):

  entry point                   shapes (N, K) covered
  esme_hip_dequantize_4bit_t    (1, 64) the smallest; (65, 128) one row past a 16-byte slot and a tile tail; (136, 64) a tile tail in whole slots,
                                also against contiguous tensors; (72, 128) with an explicit pitch of 512 and a lead of 72 columns
  esme_hip_dequantize_8bit_t    (1, 8) the smallest; (65, 72) tails in both directions; (136, 64); (72, 128) with the explicit pitch
"""
import ctypes

import pytest
import torch

import footprint as fp
import test_footprint_gpu as G
from footprint import Case, Operand

pytestmark = pytest.mark.gpu
DEV = G.DEV
CASES = []


def add(id, symbols, build, plain):
    spec = G.Spec(id, tuple('esme_hip_' + s for s in symbols.split()), build)
    spec.plain = plain
    CASES.append(spec)


def dequant_t_case(bits, N, K, ld=None, lead=None):
    g = torch.Generator().manual_seed(N + K + bits)
    o = Operand('out', torch.empty((K, N), dtype=G.BF), 'out', ld=ld, lead=lead)
    if bits == 4:
        cb = (ctypes.c_float * 16)(*G.CODEBOOK)
        ops = [Operand('codes', torch.randint(0, 256, (N, K // 2), generator=g).to(torch.uint8), pad=False),
               Operand('absmax', torch.rand(N, K // 64, generator=g), pad=False), o]

        def call(v):
            G.call_c('esme_hip_dequantize_4bit_t', G.P(v['codes']), G.P(v['absmax']), N, K, cb, G.P(v['out']), max(v['out'].stride(0), N))
    else:
        ops = [Operand('codes', torch.randint(-127, 128, (N, K), generator=g).to(torch.int8), pad=False), Operand('scale', torch.rand(N, generator=g)), o]

        def call(v):
            G.call_c('esme_hip_dequantize_8bit_t', G.P(v['codes']), G.P(v['scale']), N, K, G.P(v['out']), max(v['out'].stride(0), N))
    return Case(f'dequantize_{bits}bit_t {N}x{K}', ops, call)


for _bits, _shapes in ((4, [(1, 64), (65, 128), (136, 64)]), (8, [(1, 8), (65, 72), (136, 64)])):
    for _N, _K in _shapes:
        add(f'dequantize_{_bits}bit_t-{_N}x{_K}', f'dequantize_{_bits}bit_t', lambda b=_bits, N=_N, K=_K: dequant_t_case(b, N, K), _N % 8 == 0)
    add(f'dequantize_{_bits}bit_t-72x128-ld512', f'dequantize_{_bits}bit_t', lambda b=_bits: dequant_t_case(b, 72, 128, ld=512, lead=72), True)


@pytest.mark.parametrize('spec', CASES, ids=[c.id for c in CASES])
def test_dequant_t_footprint(spec, monkeypatch):
    from esme import _hip, _hip_dequant_t
    lib, called = _hip.load(), set()
    _hip_dequant_t.bind(lib)                 # (typed on the handle itself: the recorder below hands out plain wrappers)

    class Recorder:
        """The loaded library with every esme_hip_* call noted: the case must reach the entry point its coverage label names."""
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
    res = fp.check(case, DEV, plain=spec.plain)   # (a contiguous (K, N) out with N % 8 != 0 is not a legal operand: ldo % 8 == 0)
    monkeypatch.undo()
    assert set(spec.symbols) <= called, f'{spec.id}: labelled {sorted(spec.symbols)}, but the run called {sorted(called)}'
    out = res['nan'].outputs['out'].view(torch.bfloat16).float()
    assert bool(torch.isfinite(out).all()) and bool(out.any()), f'{case.name}: out was not written everywhere'
