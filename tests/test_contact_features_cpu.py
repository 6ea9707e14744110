"""Contact-regression features and ContactHead.fit without a GPU: the error bound of tests/contact_feature_bounds.py accepts a float32
emulation of contact_gather_kernel and rejects every defect the emulation can switch on; the bookkeeping of
include/esme_hip_contact_features.h (binding table, exported symbols, footprint coverage, host-side argument checks); the L1 logistic
regression of ContactHead.fit on a planted problem (KKT residual recomputed here in float64); fit_contact_head's label handling."""
import ctypes
import math
import os
import re
import warnings

import pytest
import torch

import contact_feature_bounds as FB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'esme_hip_contact_features.h')
LENGTHS = (0, 1, 2, 3, 18, 66, 67, 130, 195)
H, D = 3, 64
_SHARED = {}


def _case(qp):
    """One batch and pair list, its float64 reference and bound: computed once per q_prescaled, shared, never modified."""
    if qp not in _SHARED:
        layers, cu, scale = FB.make_operands(LENGTHS, H, D, seed=1, qp=qp)
        pairs = FB.make_pairs(LENGTHS, seed=2)
        _SHARED[qp] = dict(layers=layers, cu=cu, scale=scale, pairs=pairs, ref=FB.reference_features(layers, cu, H, D, scale, pairs),
                           bound=FB.feature_bound(layers, cu, H, D, scale, pairs))
    return _SHARED[qp]


def _worst(got, c):
    return float(((got.double() - c['ref']).abs() / c['bound']).max())


def test_pair_list_and_reference_shape():
    c = _case(False)
    p = c['pairs'].long()
    assert c['ref'].shape == (p.shape[0], 2 * H) and bool(torch.isfinite(c['ref']).all()) and bool((c['bound'] > 0).all())
    assert sorted(p[:, 0].unique().tolist()) == [3, 4, 5, 6, 7, 8]                   # every sequence with a kept residue
    assert bool((p[:, 1] == p[:, 2]).any()) and bool((p[:, 1] > p[:, 2]).any()) and bool((p[:, 1] < p[:, 2]).any())
    assert p.unique(dim=0).shape[0] < p.shape[0]                                     # duplicates
    # n = 1: Y = 2 A, r = t = 2 A, N = 0
    one = (p[:, 0] == 3).nonzero().reshape(-1)
    assert one.numel() and float(c['ref'][one].abs().max()) < 1e-15
    # (i, j) and (j, i) are the same number
    ref = {tuple(r): v for r, v in zip(p.tolist(), c['ref'])}
    swapped = [(s, i, j) for s, i, j in ref if i != j and (s, j, i) in ref]
    assert swapped and all(torch.allclose(ref[s, i, j], ref[s, j, i], rtol=0, atol=1e-15) for s, i, j in swapped)


@pytest.mark.parametrize('qp', [False, True], ids=['scaled-in-kernel', 'q-prescaled'])
def test_bound_accepts_the_correct_emulation(qp):
    c = _case(qp)
    got = FB.emulate_features(c['layers'], c['cu'], H, D, c['scale'], c['pairs'])
    worst = _worst(got, c)
    print(f'correct emulation: worst err / bound {worst:.3f}')
    assert worst <= 1.0
    assert float(c['ref'].abs().max()) >= 100 * float(c['bound'].max())              # the signal stands far above the bound


@pytest.mark.parametrize('qp', [False, True], ids=['scaled-in-kernel', 'q-prescaled'])
@pytest.mark.parametrize('defect', FB.DEFECTS)
def test_bound_rejects_every_defect(defect, qp):
    c = _case(qp)
    got = FB.emulate_features(c['layers'], c['cu'], H, D, c['scale'], c['pairs'], defect=defect)
    worst = _worst(got, c)
    print(f'{defect}: worst err / bound {worst:.1f}')
    assert worst > 1.0, f'the bound accepts the defect {defect!r}'


# ------------------------------------------------------------------ the header's bookkeeping

def _declared(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r'\b(esme_hip_\w+)\s*\(([^;{}]*?)\)\s*;', text)}


def test_header_symbols_exported_and_bound():
    from esme import _hip, _hip_contact_features as HF, _hip_contacts
    declared = set(_declared())
    assert declared == set(HF.SIGNATURES) == {'esme_hip_contact_features_workspace_bytes', 'esme_hip_contact_features'}
    lib = ctypes.CDLL(_hip.lib_path())
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/esme_hip_contact_features.h but not exported'
    for name, args in _declared().items():
        assert len([a for a in args.split(',') if a.strip()]) == len(HF.SIGNATURES[name][1]), name
    # the other two headers and tables keep their own symbols
    assert not declared & set(_hip.SIGNATURES) and not declared & set(_hip_contacts.SIGNATURES)
    for other in ('esme_hip.h', 'esme_hip_contacts.h'):
        assert not declared & set(_declared(os.path.join(ROOT, 'include', other))), other
        assert 'esme_hip_contact_features' not in open(os.path.join(ROOT, 'include', other)).read()


def test_every_pointer_entry_point_has_a_footprint_case():
    import test_contact_features_footprint_gpu as G
    names = [n for n, args in _declared().items() if '*' in args]
    assert names == ['esme_hip_contact_features']
    covered = {s for c in G.CASES for s in c.symbols}
    for n in names:
        assert n in covered, f'{n}: no case in tests/test_contact_features_footprint_gpu.py names it'
        assert re.search(rf'\b{n}\b', G.__doc__), f'{n}: missing from the docstring of tests/test_contact_features_footprint_gpu.py'
    assert covered <= set(_declared()), covered - set(_declared())
    ids = [c.id for c in G.CASES]
    assert len(ids) == len(set(ids))


def test_workspace_formula_and_argument_checks():
    """Host-side checks need no device: the size query's stated formula, the no-ops and the argument errors that return before any launch."""
    from esme import _hip_contact_features as HF
    assert HF.workspace_bytes(7, 1000, 20) == (3 * 20 * 1000 + 20 * 7) * 4
    assert HF.workspace_bytes(0, 0, 1) == 0
    with pytest.raises(RuntimeError, match='bad sizes'):
        HF.workspace_bytes(1, 10, 0)
    lib = HF._lib()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    args = dict(q=p, k=p, ld=64, cu=p, B=1, T=8, H=2, d=32, max_len=8, scale=0.1, qp=0, f=1, e=1, pairs=p, P=4, feat=p, ldf=6, col0=4, ws=p, nb=1 << 20, stream=None)
    call = lambda **kw: lib.esme_hip_contact_features(*{**args, **kw}.values())
    assert call(d=48, H=1) == -2 and b'head dim' in lib.esme_hip_last_error()
    assert call(ld=60) == -1 and call(q=p + 2) == -1 and call(nb=8) == -1 and call(pairs=None) == -1 and call(feat=None) == -1
    assert call(ldf=5) == -1 and b'ld_feat' in lib.esme_hip_last_error()
    assert call(col0=-1) == -1 and call(P=-1) == -1 and call(P=1 << 31) == -1 and call(feat=p + 2) == -1
    assert call(max_len=1 << 27, ld=64) == -2 and b'ESME_HIP_CONTACT_MAX_SEQ_ELEMS' in lib.esme_hip_last_error()
    assert call(B=0) == 0 and call(T=0) == 0 and call(P=0) == 0 and call(P=0, pairs=None, feat=None) == 0      # nothing to do: no launch


# ------------------------------------------------------------------ ContactHead.fit

P_FIT, K_FIT, C_FIT, TOL = 4000, 12, 0.15, 1e-6


def _planted():
    """P = 4 000 pairs, 12 columns whose scales spread over 1e-3 .. 1 (with non-zero means), Bernoulli labels of a sparse (w*, b*)."""
    if 'fit' not in _SHARED:
        g = torch.Generator().manual_seed(0)
        scales = torch.logspace(-3, 0, K_FIT, dtype=torch.float64)
        X = torch.randn(P_FIT, K_FIT, generator=g, dtype=torch.float64) * scales + 0.3 * scales
        w = torch.zeros(K_FIT, dtype=torch.float64)
        w[[2, 7, 10, 11]] = torch.tensor([40.0, -6.0, 2.5, -1.5], dtype=torch.float64)
        b = -1.0
        y = (torch.rand(P_FIT, generator=g, dtype=torch.float64) < torch.sigmoid(X @ w + b)).double()
        _SHARED['fit'] = (X.float(), y, w, b)             # (features are float32, as contact_features returns them)
    return _SHARED['fit']


def _objective(X, y, w, b, lam):
    z = X.double() @ w + b
    return float((torch.nn.functional.softplus(z) - y * z).mean() + lam * w.abs().sum())


def _kkt(X, y, w, b, lam):
    """The KKT residual of the issue, with sums of its own (a float64 matrix-vector product over the transposed copy)."""
    X64 = X.double()
    z = (X64 * w).sum(1) + b
    r = torch.sigmoid(z) - y
    g = (X64.T.contiguous() * r).sum(1) / X.shape[0]
    gb = float(r.mean())
    at = torch.where(w != 0, (g + lam * torch.sign(w)).abs(), (g.abs() - lam).clamp(min=0))
    return max(abs(gb), float(at.max()))


def test_fit_meets_its_kkt_contract():
    from esme import ContactHead
    X, y, w_star, b_star = _planted()
    lam = 1.0 / (C_FIT * P_FIT)
    with warnings.catch_warnings():
        warnings.simplefilter('error')                      # converges within the default max_iter: no ConvergenceWarning
        head = ContactHead.fit(X, y, 3, 4, C=C_FIT, tol=TOL)
    info = head.fit_info
    w, b = info['weight'], info['bias']
    res = _kkt(X, y, w, b, lam)
    print(f"iterations {info['iterations']}, residual {info['residual']:.3e} (recomputed {res:.3e}), objective {info['objective']:.9f}")
    assert w.dtype == torch.float64 and info['converged'] and info['residual'] <= TOL
    assert res <= 2 * TOL
    F = _objective(X, y, w, b, lam)
    assert abs(F - info['objective']) <= 1e-12
    assert F <= _objective(X, y, w_star, b_star, lam)
    assert F <= _objective(X, y, torch.zeros(K_FIT, dtype=torch.float64), math.log(float(y.mean()) / (1 - float(y.mean()))), lam)
    assert 0 < int((w != 0).sum()) < K_FIT                # the L1 term removes columns, and not all of them
    # the head stores the float32 rounding, in the original feature units
    assert torch.equal(head.regression.weight, w.float().reshape(1, -1)) and float(head.regression.bias) == float(torch.tensor(b).float())
    assert (head.num_layers, head.attention_heads) == (3, 4) and head.regression.weight.dtype == torch.float32

    again = ContactHead.fit(X, y, 3, 4, C=C_FIT, tol=TOL)
    assert torch.equal(again.fit_info['weight'], w) and again.fit_info['bias'] == b and again.fit_info['iterations'] == info['iterations']
    ones = ContactHead.fit(X, y, 3, 4, C=C_FIT, tol=TOL, sample_weight=torch.ones(P_FIT))
    assert torch.equal(ones.fit_info['weight'], w) and ones.fit_info['bias'] == b


def test_fit_warns_when_it_stops_early_and_rejects_bad_input():
    from esme import ContactHead
    X, y, _, _ = _planted()
    with pytest.warns(UserWarning, match='ConvergenceWarning'):
        head = ContactHead.fit(X, y, 3, 4, tol=1e-12, max_iter=3)
    assert head.fit_info['iterations'] == 3 and not head.fit_info['converged'] and head.fit_info['residual'] > 1e-12
    with pytest.raises(ValueError, match='one class'):
        ContactHead.fit(X, torch.ones(P_FIT), 3, 4)
    with pytest.raises(ValueError, match='one class'):
        ContactHead.fit(X, torch.zeros(P_FIT), 3, 4)
    with pytest.raises(ValueError, match='P == 0'):
        ContactHead.fit(X[:0], y[:0], 3, 4)
    with pytest.raises(ValueError, match='3 \\* 5'):
        ContactHead.fit(X, y, 3, 5)
    bad = X.clone()
    bad[7, 3] = float('nan')
    with pytest.raises(ValueError, match='non-finite'):
        ContactHead.fit(bad, y, 3, 4)


def test_fitted_head_round_trips_into_a_model():
    from esme import ESM2, ContactHead
    X, y, _, _ = _planted()
    head = ContactHead.fit(X, y, 3, 4, tol=TOL)
    again = ContactHead.load(head.state_dict(), 3, 4)
    assert torch.equal(again.regression.weight, head.regression.weight) and torch.equal(again.regression.bias, head.regression.bias)
    model = ESM2(num_layers=3, embed_dim=64, attention_heads=4)
    model.set_contact_head(again)
    assert torch.equal(model.contact_head.regression.weight, head.regression.weight)
    assert 'contact_head.regression.weight' in model.state_dict()


# ------------------------------------------------------------------ fit_contact_head

class _Stub:
    """A model whose contact_features returns fixed tensors: 2 proteins of 9 and 7 residues, every i < j, planted features."""
    attention_heads = 2

    def __init__(self):
        from esme.contacts import all_pairs
        self.layers = [None, None]
        self.n = [9, 7]
        self.pairs = all_pairs(self.n, 0)
        g = torch.Generator().manual_seed(3)
        self.X = torch.randn(self.pairs.shape[0], 4, generator=g)
        self.asked = []

    def contact_features(self, tokens, pad_args=None, pairs=None, min_sep=0, lora_names=None):
        self.asked.append(min_sep)
        return self.X, self.pairs

    def maps(self):
        g = torch.Generator().manual_seed(4)
        out = []
        for s, n in enumerate(self.n):
            sel = self.pairs[:, 0] == s
            z = 2.0 * self.X[sel, 0] - 1.0 * self.X[sel, 3]
            m = torch.full((n, n), -1.0)
            i, j = self.pairs[sel, 1].long(), self.pairs[sel, 2].long()
            m[i, j] = (torch.rand(z.shape, generator=g) < torch.sigmoid(z)).float()
            out.append(m)
        out[0][2, :] = -1                                  # residue 2 of protein 0 is unresolved
        out[0][:, 2] = -1
        return out


def test_fit_contact_head_labels_min_sep_and_subsampling(monkeypatch):
    from esme import ContactHead, contacts, fit_contact_head
    stub = _Stub()
    maps = stub.maps()
    batch = [(torch.zeros(20, dtype=torch.long), (torch.tensor([0, 11, 20], dtype=torch.int32), 11))]
    seen = []
    real = ContactHead.fit.__func__

    def spy(cls, X, y, L, Hh, **kw):
        seen.append((X.clone(), y.clone(), L, Hh, kw))
        return real(cls, X, y, L, Hh, **kw)
    monkeypatch.setattr(contacts.ContactHead, 'fit', classmethod(spy))

    head = fit_contact_head(stub, batch, maps, min_sep=3, tol=1e-5)
    assert isinstance(head, ContactHead) and (head.num_layers, head.attention_heads) == (2, 2) and stub.asked == [3]
    X, y, L, Hh, kw = seen[-1]
    assert (L, Hh, kw) == (2, 2, {'tol': 1e-5})
    p = stub.pairs.long()
    want = [r for r in range(p.shape[0]) if p[r, 2] - p[r, 1] >= 3 and not (p[r, 0] == 0 and 2 in (int(p[r, 1]), int(p[r, 2])))]
    assert len(want) < p.shape[0] and torch.equal(X, stub.X[want])                   # min_sep honoured, the unlabelled pairs dropped
    assert torch.equal(y, torch.stack([maps[int(p[r, 0])][p[r, 1], p[r, 2]] for r in want])) and bool(((y == 0) | (y == 1)).all())

    fit_contact_head(stub, batch, maps, min_sep=3, max_pairs=10, seed=5)
    a = seen[-1]
    fit_contact_head(stub, batch, maps, min_sep=3, max_pairs=10, seed=5)
    b = seen[-1]
    fit_contact_head(stub, batch, maps, min_sep=3, max_pairs=10, seed=6)
    c = seen[-1]
    assert a[0].shape == (10, 4) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], c[0])
    rows = {tuple(r.tolist()) for r in stub.X[want]}
    assert all(tuple(r.tolist()) in rows for r in a[0])                              # a subset of the labelled pairs
    with pytest.raises(ValueError, match='contact maps'):
        fit_contact_head(stub, batch, maps[:1])


def test_contact_features_public_surface():
    import esme
    from esme import ESM2
    assert {'ContactFeatureAccumulator', 'fit_contact_head', 'ContactHead'} <= set(esme.__all__)
    model = ESM2(num_layers=1, embed_dim=64, attention_heads=4)
    assert model.contact_head is None
    with pytest.raises(NotImplementedError, match='contact_features'):
        model.graphed(torch.zeros(4, dtype=torch.long), (torch.tensor([0, 4], dtype=torch.int32), 4), what='contact_features')
    from esme.contacts import all_pairs, check_pairs
    assert all_pairs([4, 0, 3], 2).tolist() == [[0, 0, 2], [0, 0, 3], [0, 1, 3], [2, 0, 2]]
    assert all_pairs([3], 0).tolist() == [[0, 0, 1], [0, 0, 2], [0, 1, 2]] and all_pairs([1, 0], 0).shape == (0, 3)
    got = check_pairs([torch.tensor([[0, 3], [2, 2]]), torch.zeros(0, 2, dtype=torch.long), torch.tensor([[1, 0]])], [4, 0, 3], 'cpu')
    assert got.dtype == torch.int32 and got.tolist() == [[0, 0, 3], [0, 2, 2], [2, 1, 0]]
    for bad in ([[0, 0, 4]], [[1, 0, 0]], [[3, 0, 0]], [[0, -1, 0]], [[-1, 0, 0]]):
        with pytest.raises(ValueError, match='out of range'):
            check_pairs(torch.tensor(bad), [4, 0, 3], 'cpu')
    with pytest.raises(ValueError, match='integer'):
        check_pairs(torch.zeros(2, 3), [4, 0, 3], 'cpu')
