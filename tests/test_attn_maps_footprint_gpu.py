"""The device-pointer entry point of include/esme_hip_attn_maps.h inside guard-banded arenas (tests/footprint.py): write containment, read
independence (NaN against zero guards), layout invariance (arena views against contiguous tensors) and an uninitialised, exact-size
workspace -- the discipline tests/test_footprint_gpu.py applies to include/esme_hip.h, with a case list of its own.

Coverage (tests/test_attn_maps_cpu.py fails when a pointer entry point of the header has no case here):

  entry point                      forms covered
  esme_hip_attn_maps               head dims 32 / 64, with and without head weights, fp32 and bf16 output; q / k padded column blocks of one
                                   (T, 3E) arena; cu_lens, head_list, head_weights, map_off and the exact-size workspace
                                   (esme_hip_attn_maps_workspace_bytes) in arenas of their own; the map an 'inout' operand filled with a
                                   sentinel: three slots per sequence of which the call owns slots 1 .. (slot0 = 1), and a gap between the
                                   runs of neighbouring sequences -- slot 0, the unowned slots and the gaps keep the sentinel, every owned
                                   element loses it; lengths 1, 64, 65, 130
"""
import pytest
import torch

import attn_map_bounds as MB
import footprint as fp
import test_footprint_gpu as G
from footprint import Case, Operand

pytestmark = pytest.mark.gpu
DEV = G.DEV
LENGTHS = (1, 64, 65, 130)
H, HEADS, SLOTS, SLOT0, GAP, SENTINEL = 3, [2, 0], 3, 1, 37, -7.0
CASES = []


def add(id, symbols, build):
    CASES.append(G.Spec(id, tuple('esme_hip_' + s for s in symbols.split()), build))


def layout(weighted):
    """(map_off, owned mask, total): SLOTS blocks per sequence and GAP elements between the runs; the call owns slots SLOT0 .. of each."""
    n_out = 1 if weighted else len(HEADS)
    off, owned, pos = [], [], GAP
    for S in LENGTHS:
        off.append(pos)
        pos += SLOTS * S * S + GAP
    mask = torch.zeros(pos, dtype=torch.bool)
    for o, S in zip(off, LENGTHS):
        mask[o + SLOT0 * S * S:o + (SLOT0 + n_out) * S * S] = True
    return torch.tensor(off, dtype=torch.int64), mask, pos


def maps_case(d, weighted, bf16):
    from esme import _hip_attn_maps as HM
    layers, cu, scale = MB.make_operands(LENGTHS, H, d, seed=7 + d)
    q, k, _ = layers[0]
    T, E, B, n = int(cu[-1]), H * d, len(LENGTHS), len(HEADS)
    off, mask, total = layout(weighted)
    dt = torch.bfloat16 if bf16 else torch.float32
    nbytes = HM.workspace_bytes(B, T, n)
    ops = [Operand('qkv', torch.cat((q, k, torch.zeros(T, E, dtype=G.BF)), 1).contiguous()), Operand('cu_lens', cu),
           Operand('head_list', torch.tensor(HEADS, dtype=torch.int32)), Operand('head_weights', torch.tensor([0.25, 0.5])),
           Operand('map_off', off), Operand('ws', torch.empty(nbytes, dtype=torch.uint8), 'ws'),
           Operand('map', torch.full((total,), SENTINEL, dtype=dt), 'inout')]

    def call(v):
        qkv = v['qkv']
        G.call_c('esme_hip_attn_maps', G.P(qkv), G.P(qkv) + 2 * E, qkv.stride(0), G.P(v['cu_lens']), B, T, H, d, max(LENGTHS), scale, 0,
                 G.P(v['head_list']), n, G.P(v['head_weights']) if weighted else None, G.P(v['map']), int(bf16), G.P(v['map_off']), SLOT0,
                 G.P(v['ws']), nbytes)
    case = Case(f'attn_maps d{d} weighted{int(weighted)} bf16{int(bf16)}', ops, call)
    case.owned, case.dtype = mask, dt
    return case


for _d in (32, 64):
    for _w in (False, True):
        for _b in (False, True):
            add(f'attn_maps-d{_d}-{"weighted" if _w else "heads"}-{"bf16" if _b else "fp32"}', 'attn_maps attn_maps_workspace_bytes',
                lambda d=_d, w=_w, b=_b: maps_case(d, w, b))


@pytest.mark.parametrize('spec', CASES, ids=[c.id for c in CASES])
def test_attn_maps_footprint(spec, monkeypatch):
    from esme import _hip, _hip_attn_maps
    lib, called = _hip.load(), set()
    _hip_attn_maps.bind(lib)                 # (typed on the handle itself: the recorder below hands out plain wrappers)

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
    # the gaps of the 'inout' map: slot 0, the unowned slots and the elements between the sequences' runs keep the sentinel; every owned
    # element is a finite value of [0, 1] (the weights are positive and sum to less than 1), so none keeps it
    for fill in ('nan', 'zero', 'plain'):
        got = res[fill].outputs['map'].view(case.dtype).reshape(-1).float()
        assert bool((got[~case.owned] == SENTINEL).all()), f'{case.name} [{fill}]: an element outside the owned blocks was written'
        own = got[case.owned]
        assert bool(torch.isfinite(own).all()) and float(own.min()) >= 0 and float(own.max()) <= 1.0 + 2 ** -7, f'{case.name} [{fill}]: owned elements'
