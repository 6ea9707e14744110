"""The launches of an FFN branch with LoRA adapters inside guard-banded arenas (tests/footprint.py): write containment, read independence
(NaN guards against zero guards) and layout invariance, the discipline tests/test_footprint_gpu.py applies to include/esme_hip.h, with a
case list of its own for the shapes the FFN adapters bring (E = 128, F = 512, X = 64):

  esme_hip_lora_down        K = F = 512, x = the first F columns of the (T, F + X) buffer `mid` (ldx = F + X and the arena's pads), u = its last
                            X columns; rank 24 of 64: the activation columns stay as they are, the columns past the rank become zero
  esme_hip_lora_down_ln     K = E next to the stream, on the FFN LayerNorm's statistics (as for the QKV GEMM)
  esme_hip_gemm_bf16_fused  the LayerNorm-folded up GEMM over K = E + X with the GELU / SwiGLU epilogue, writing a column view of `mid`
                            (ldc = F + X: the extension columns next to it are not its to write); the residual GEMM over K = F + X with
                            row statistics
Each as a launch of its own, and the four chained as FlashTransformerLayer._ffn_lora issues them.  T = 1 and 257 (a ragged last row tile
of the 128- and 256-row kernels)."""
import pytest
import torch

import footprint as fp
import test_footprint_gpu as G
from footprint import Case, Operand

pytestmark = pytest.mark.gpu
DEV = G.DEV
E, FF, X, RANK = 128, 512, 64, 24
CASES = []


def add(id, symbols, build):
    CASES.append(G.Spec(id, tuple('esme_hip_' + s for s in symbols.split()), build))


def ffn_case(kind, T, swiglu=False):
    from esme import _hip
    N_up = 2 * FF if swiglu else FF
    epi = _hip.EPI_SWIGLU if swiglu else _hip.EPI_GELU
    xu = torch.cat((G.rnd((T, E), 1), G.rnd((T, X), 2)), 1).contiguous()
    x = xu[:, :E].double()
    ops = {'xu': Operand('xu', xu, 'inout'),
           'A_up': Operand('A_up', G.rnd((RANK, E), 3, E ** -0.5), pad=False),
           'sums': Operand('sums', torch.stack((x.sum(1), (x * x).sum(1)), 1).float(), pad=False),
           'c1A': Operand('c1A', G.rnd((RANK,), 4, 1.0, G.F32)), 'bA': Operand('bA', G.rnd((RANK,), 5, 1.0, G.F32)),
           'W_up': Operand('W_up', G.rnd((N_up, E + X), 6, E ** -0.5), pad=False),
           'c1': Operand('c1', G.rnd((N_up,), 7, 1.0, G.F32)), 'c2': Operand('c2', G.rnd((N_up,), 8, 1.0, G.F32)),
           'mid': Operand('mid', G.rnd((T, FF + X), 9), 'inout'),
           'A_down': Operand('A_down', G.rnd((RANK, FF), 10, FF ** -0.5), pad=False),
           'W_down': Operand('W_down', G.rnd((E, FF + X), 11, FF ** -0.5), pad=False),
           'bias': Operand('bias', G.rnd((E,), 12, 0.5)), 'resid': Operand('resid', G.rnd((T, E), 13)), 'C': G.out('C', (T, E))}

    def down_ln(v):
        _hip.lora_down(v['xu'][:, :E], v['A_up'], v['xu'][:, E:], ln=(v['sums'].view(1, T, 2), E, 1e-5, v['c1A'], v['bA']))

    def up(v):
        _hip.gemm_fused(v['xu'], v['W_up'], None, epi, out=v['mid'][:, :FF], ln=(v['sums'].view(1, T, 2), E, 1e-5, v['c1'], v['c2'], None))

    def down(v):
        _hip.lora_down(v['mid'][:, :FF], v['A_down'], v['mid'][:, FF:])

    def resid(v):
        _hip.gemm_fused(v['mid'], v['W_down'], v['bias'], _hip.EPI_RESIDUAL, resid=v['resid'], alpha=0.75, out=v['C'], stats_out=v['stats'])

    steps = {'lora_down_ln': (down_ln, 'xu A_up sums c1A bA'), 'up': (up, 'xu W_up sums c1 c2 mid'), 'lora_down': (down, 'mid A_down'),
             'residual': (resid, 'mid W_down bias resid C'), 'chain': (None, ' '.join(ops))}
    fn, names = steps[kind]
    used = [ops[n] for n in names.split()]
    if kind in ('residual', 'chain'):
        used.append(G.out('stats', (_hip.stats_blocks(T, E) * T, 2), G.F32, pad=False))

    def call(v):
        for f in ((down_ln, up, down, resid) if kind == 'chain' else (fn,)):
            f(v)
    return Case(f"ffn lora {kind} {'swiglu' if swiglu else 'gelu'} T{T}", used, call)


for _T in (1, 257):
    add(f'lora_down-K512-T{_T}', 'lora_down', lambda T=_T: ffn_case('lora_down', T))
    add(f'lora_down_ln-ffn-T{_T}', 'lora_down_ln', lambda T=_T: ffn_case('lora_down_ln', T))
    add(f'residual-K576-T{_T}', 'gemm_bf16_fused', lambda T=_T: ffn_case('residual', T))
    for _sw in (False, True):
        _n = 'swiglu' if _sw else 'gelu'
        add(f'up-{_n}-K192-T{_T}', 'gemm_bf16_fused', lambda T=_T, sw=_sw: ffn_case('up', T, sw))
        add(f'chain-{_n}-T{_T}', 'lora_down lora_down_ln gemm_bf16_fused', lambda T=_T, sw=_sw: ffn_case('chain', T, sw))


@pytest.mark.parametrize('spec', CASES, ids=[c.id for c in CASES])
def test_ffn_lora_footprint(spec, monkeypatch):
    from esme import _hip
    lib, called = _hip.load(), set()

    class Recorder:
        """The loaded library with every esme_hip_* call noted: the case must reach the entry points its label names."""
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
    for op in case.operands:
        if op.role in ('out', 'inout') and op.data.dtype.is_floating_point:
            assert bool(torch.isfinite(res['nan'].outputs[op.name].view(op.data.dtype).float()).all()), f'{case.name}: {op.name} is not finite'
    if 'lora_down' in spec.id or 'chain' in spec.id:                  # the down-projection's own contract on `mid`
        mid = res['nan'].outputs['mid'].view(torch.bfloat16) if 'mid' in res['nan'].outputs else None
        if mid is not None:
            assert not bool(mid[:, FF + RANK:].any()), 'columns past the rank are zero'
            assert bool(mid[:, FF:FF + RANK].any())
