"""The device-pointer entry point of include/esme_hip_contact_features.h inside guard-banded arenas (tests/footprint.py): write
containment, read independence (NaN against zero guards), layout invariance (arena views against contiguous tensors) and an
uninitialised, exact-size workspace -- the discipline tests/test_contacts_footprint_gpu.py applies to include/esme_hip_contacts.h, with a
case list of its own.

Coverage (tests/test_contact_features_cpu.py fails when a pointer entry point of the header has no case here):

  entry point                      forms covered
  esme_hip_contact_features        head dims 16 / 32 / 64 / 128, q_prescaled 0 / 1; q / k column views of one (T, 3E) arena; cu_lens, the pair list and
                                   the exact-size workspace (esme_hip_contact_features_workspace_bytes) in arenas of their own; feat an output of
                                   L H columns inside a wider row (ld_feat > L H: the padding columns are guard), two layers through col0;
                                   lengths 0, 0, 1, 2, 3, 18, 66, 67, 130, 195, 0 (empty sequences first and last); pairs with i < j, i == j,
                                   i > j, duplicates, shuffled
"""
import pytest
import torch

import contact_feature_bounds as FB
import footprint as fp
import test_footprint_gpu as G
from footprint import Case, Operand

pytestmark = pytest.mark.gpu
DEV = G.DEV
LENGTHS = (0, 0, 1, 2, 3, 18, 66, 67, 130, 195, 0)
CASES = []


def add(id, symbols, build):
    CASES.append(G.Spec(id, tuple('esme_hip_' + s for s in symbols.split()), build))


def features_case(H, d, qp):
    from esme import _hip_contact_features as HF
    layers, cu, scale = FB.make_operands(LENGTHS, H, d, seed=9 + d, qp=bool(qp))
    T, E, B = int(cu[-1]), H * d, len(LENGTHS)
    pairs = FB.make_pairs(LENGTHS, seed=d, random_pairs=60)
    P = pairs.shape[0]
    nbytes = HF.workspace_bytes(B, T, H)
    ops = [Operand(f'qkv{l}', torch.cat((q, k, torch.zeros(T, E, dtype=G.BF)), 1).contiguous()) for l, (q, k, _) in enumerate(layers)]
    ops += [Operand('cu_lens', cu), Operand('pairs', pairs.reshape(-1)), Operand('ws', torch.empty(nbytes, dtype=torch.uint8), 'ws'),
            G.out('feat', (P, 2 * H), G.F32)]

    def call(v):
        for l in range(2):
            qkv, feat = v[f'qkv{l}'], v['feat']
            G.call_c('esme_hip_contact_features', G.P(qkv), G.P(qkv) + 2 * E, qkv.stride(0), G.P(v['cu_lens']), B, T, H, d, max(LENGTHS), scale, qp, 1, 1,
                     G.P(v['pairs']), P, G.P(feat), feat.stride(0), l * H, G.P(v['ws']), nbytes)
    return Case(f'contact_features H{H} d{d} qp{qp}', ops, call)


for _H, _d, _qp in [(20, 16, 0), (5, 32, 1), (3, 64, 1), (3, 64, 0), (2, 128, 0)]:
    add(f'contact_features-H{_H}-d{_d}-qp{_qp}', 'contact_features contact_features_workspace_bytes', lambda H=_H, d=_d, qp=_qp: features_case(H, d, qp))


@pytest.mark.parametrize('spec', CASES, ids=[c.id for c in CASES])
def test_contact_features_footprint(spec, monkeypatch):
    from esme import _hip, _hip_contact_features
    lib, called = _hip.load(), set()
    _hip_contact_features.bind(lib)          # (typed on the handle itself: the recorder below hands out plain wrappers)

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
    feat = [op for op in case.operands if op.name == 'feat'][0]
    res = fp.check(case, DEV)
    monkeypatch.undo()
    assert set(spec.symbols) <= called, f'{spec.id}: labelled {sorted(spec.symbols)}, but the run called {sorted(called)}'
    # the case itself is sound: every feature is finite (an unwritten element or a NaN row of an out-of-range pair would show) and the
    # row pitch of the arena is wider than the matrix
    out = res['nan'].outputs['feat'].view(torch.float32)
    assert out.shape == tuple(feat.data.shape) and bool(torch.isfinite(out).all()), f'{case.name}: feat is not finite'
    assert fp.Arena(feat, 'zero', 'cpu').ld > feat.cols
