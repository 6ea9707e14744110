"""Contact prediction without a GPU: the error bound of tests/contact_bounds.py accepts a float32 emulation of the kernel and rejects
every defect the emulation can switch on; an analytic case; ContactHead loading; the model's public surface; and the bookkeeping of the
new header (footprint coverage, binding table, exported symbols)."""
import ctypes
import os
import re

import pytest
import torch

import contact_bounds as CB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'esme_hip_contacts.h')
LENGTHS = (0, 1, 2, 3, 18, 66, 67, 130, 195)
H, D, BIAS = 3, 64, -0.75
_SHARED = {}


def _case():
    """One batch, its float64 reference and bound: computed once, shared, never modified."""
    if not _SHARED:
        layers, cu, scale = CB.make_operands(LENGTHS, H, D, seed=1)
        w = torch.randn(2, H, generator=torch.Generator().manual_seed(5))
        ref = CB.reference_contacts(layers, cu, H, D, scale, w, BIAS)
        bound = CB.contact_bound(layers, cu, H, D, scale, w, BIAS)
        _SHARED.update(layers=layers, cu=cu, scale=scale, w=w, ref=ref, bound=bound)
    return _SHARED


def _worst(maps, c):
    return max(float(((m.double() - r).abs() / b).max()) for m, r, b in zip(maps, c['ref'], c['bound']) if r.numel())


def test_reference_shapes_and_symmetry():
    c = _case()
    assert [r.shape[0] for r in c['ref']] == [0, 0, 0, 1, 16, 64, 65, 128, 193]
    for r in c['ref']:
        assert torch.allclose(r, r.T, rtol=0, atol=1e-12)
    # n = 1: Y = 2 A, r = t = 2 A, so N = 0 and the logit is the bias
    assert abs(float(c['ref'][3]) - BIAS) < 1e-12


def test_bound_accepts_the_correct_emulation():
    c = _case()
    got = CB.emulate_contacts(c['layers'], c['cu'], H, D, c['scale'], c['w'], BIAS)
    worst = _worst(got, c)
    print(f'correct emulation: worst err / bound {worst:.3f}')
    assert worst <= 1.0
    signal = max(float((r - BIAS).abs().max()) for r in c['ref'] if r.numel())
    assert signal >= 100 * max(float(b.max()) for b in c['bound'] if b.numel())


@pytest.mark.parametrize('defect', CB.DEFECTS)
def test_bound_rejects_every_defect(defect):
    c = _case()
    got = CB.emulate_contacts(c['layers'], c['cu'], H, D, c['scale'], c['w'], BIAS, defect=defect)
    worst = _worst(got, c)
    print(f'{defect}: worst err / bound {worst:.1f}')
    assert worst > 1.0, f'the bound accepts the defect {defect!r}'


def test_zero_queries_give_the_bias():
    """q = 0: P is uniform (1 / S), A = 1 / S, Y = 2 / S, r = 2 n / S, t = 2 n^2 / S, r r^T / t = 2 / S = Y: every logit is the bias."""
    layers, cu, scale = CB.make_operands((5, 40, 70), 2, 32, seed=2)
    zero = [(torch.zeros_like(q), k, qp) for q, k, qp in layers]
    w = torch.tensor([[1.5, -2.0], [0.25, 3.0]])
    for maps, tol in ((CB.reference_contacts(zero, cu, 2, 32, scale, w, BIAS), 1e-12), (CB.emulate_contacts(zero, cu, 2, 32, scale, w, BIAS), 1e-5)):
        for m in maps:
            assert float((m.double() - BIAS).abs().max()) < tol


def test_contact_head_load_round_trips(tmp_path):
    from esme import ContactHead
    from safetensors.torch import save_file
    L, heads = 3, 4
    w, b = torch.randn(1, L * heads), torch.randn(1)
    for state in ({'contact_head.regression.weight': w, 'contact_head.regression.bias': b},
                  {'model': {'contact_head.regression.weight': w, 'contact_head.regression.bias': b}},
                  {'regression.weight': w.to(torch.bfloat16).float(), 'regression.bias': b}):
        head = ContactHead.load(state, L, heads)
        ws = state.get('model', state)
        assert torch.equal(head.regression.weight, [v for k, v in ws.items() if k.endswith('weight')][0]) and torch.equal(head.regression.bias, b)
        assert head.regression.weight.dtype == torch.float32 and (head.num_layers, head.attention_heads) == (L, heads)
    path = str(tmp_path / 'head.safetensors')
    save_file({'contact_head.regression.weight': w, 'contact_head.regression.bias': b}, path)
    head = ContactHead.load(path, L, heads)
    assert torch.equal(head.regression.weight, w) and torch.equal(head.regression.bias, b)
    pt = str(tmp_path / 'head.pt')
    torch.save({'model': {'contact_head.regression.weight': w, 'contact_head.regression.bias': b}}, pt)
    assert torch.equal(ContactHead.load(pt, L, heads).regression.weight, w)
    again = ContactHead.load(head.state_dict(), L, heads)          # its own state dict
    assert torch.equal(again.regression.weight, w)


def test_contact_head_rejects_a_wrong_width():
    from esme import ESM2, ContactHead
    state = {'regression.weight': torch.zeros(1, 12), 'regression.bias': torch.zeros(1)}
    with pytest.raises(ValueError, match='features'):
        ContactHead.load(state, 3, 5)
    with pytest.raises(ValueError, match='regression'):
        ContactHead.load({'weight': torch.zeros(1, 12)})
    model = ESM2(num_layers=2, embed_dim=64, attention_heads=4)
    with pytest.raises(ValueError, match='does not fit'):
        model.set_contact_head(state)
    model.set_contact_head({'regression.weight': torch.ones(1, 8), 'regression.bias': torch.zeros(1)})
    assert (model.contact_head.num_layers, model.contact_head.attention_heads) == (2, 4)


def test_state_dict_keys_unchanged_without_a_head():
    from esme import ESM2
    model = ESM2(num_layers=1, embed_dim=64, attention_heads=4)
    assert model.contact_head is None
    keys = set(model.state_dict())
    assert not any('contact' in k for k in keys)
    model.set_contact_head({'regression.weight': torch.ones(1, 4), 'regression.bias': torch.zeros(1)})
    assert set(model.state_dict()) - keys == {'contact_head.regression.weight', 'contact_head.regression.bias'}


def test_predict_contacts_without_a_head_raises():
    from esme import ESM2
    model = ESM2(num_layers=1, embed_dim=64, attention_heads=4)
    with pytest.raises(RuntimeError, match='contact head'):
        model.predict_contacts(torch.zeros(4, dtype=torch.long), (torch.tensor([0, 4], dtype=torch.int32), 4))


def test_from_pretrained_picks_up_a_contact_head(tmp_path):
    from esme import ESM, synthetic as syn
    from safetensors import safe_open
    from safetensors.torch import save_file
    L, E, heads = 1, 64, 4
    path = syn.write_checkpoint(str(tmp_path / 'm.safetensors'), 'esm2_test', L, E, heads, seed=3)
    with safe_open(path, framework='pt') as f:
        state, md = {k: f.get_tensor(k) for k in f.keys()}, dict(f.metadata())
    assert ESM.from_pretrained(path).contact_head is None
    state['contact_head.regression.weight'] = torch.arange(L * heads, dtype=torch.float32).reshape(1, -1)
    state['contact_head.regression.bias'] = torch.tensor([0.5])
    save_file(state, path, metadata=md)
    head = ESM.from_pretrained(path).contact_head
    assert head is not None and torch.equal(head.regression.weight, state['contact_head.regression.weight'])


# ------------------------------------------------------------------ the header's bookkeeping

def _declared():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r'\b(esme_hip_\w+)\s*\(([^;{}]*?)\)\s*;', text)}


def test_every_pointer_entry_point_has_a_footprint_case():
    import test_contacts_footprint_gpu as G
    names = [n for n, args in _declared().items() if '*' in args]
    assert names == ['esme_hip_contact_layer']
    covered = {s for c in G.CASES for s in c.symbols}
    for n in names:
        assert n in covered, f'{n}: declared in esme_hip_contacts.h with a pointer argument, but no case in tests/test_contacts_footprint_gpu.py names it'
        assert re.search(rf'\b{n}\b', G.__doc__), f'{n}: missing from the docstring of tests/test_contacts_footprint_gpu.py'
    assert covered <= set(_declared()), covered - set(_declared())
    ids = [c.id for c in G.CASES]
    assert len(ids) == len(set(ids))


def test_header_symbols_exported_and_bound():
    from esme import _hip, _hip_contacts
    declared = set(_declared())
    assert declared == set(_hip_contacts.SIGNATURES) == {'esme_hip_contact_workspace_bytes', 'esme_hip_contact_layer'}
    lib = ctypes.CDLL(_hip.lib_path())
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/esme_hip_contacts.h but not exported'
    assert not declared & set(_hip.SIGNATURES)                                   # the main table and header keep their own symbols
    main = open(os.path.join(ROOT, 'include', 'esme_hip.h')).read()
    assert 'esme_hip_contact' not in main
    # the number of arguments of each declaration equals the binding's
    for name, args in _declared().items():
        assert len([a for a in args.split(',') if a.strip()]) == len(_hip_contacts.SIGNATURES[name][1]), name


def test_workspace_formula_and_argument_checks():
    """Host-side checks need no device: the size query's stated formula, and the argument errors that return before any launch."""
    from esme import _hip, _hip_contacts as HC
    assert HC.workspace_bytes(7, 1000, 20) == (3 * 20 * 1000 + 20 * 7) * 4
    assert HC.workspace_bytes(0, 0, 1) == 0
    with pytest.raises(RuntimeError, match='bad sizes'):
        HC.workspace_bytes(1, 10, 0)
    lib = HC._lib()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    args = dict(q=p, k=p, ld=64, cu=p, B=1, T=8, H=2, d=32, max_len=8, scale=0.1, qp=0, f=1, e=1, w=p, bias=0.0, init=1, map=p, off=p, ws=p, nb=1 << 20, stream=None)
    call = lambda **kw: lib.esme_hip_contact_layer(*{**args, **kw}.values())
    assert call(d=48, H=1) == -2 and b'head dim' in lib.esme_hip_last_error()
    assert call(ld=60) == -1 and call(q=p + 2) == -1 and call(nb=8) == -1 and call(w=None) == -1
    assert call(max_len=1 << 27, ld=64) == -2 and b'ESME_HIP_CONTACT_MAX_SEQ_ELEMS' in lib.esme_hip_last_error()
    assert call(B=0) == 0 and call(max_len=2) == 0                            # nothing to do: no launch
