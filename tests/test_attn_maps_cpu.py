"""Attention maps without a GPU: the error bound of tests/attn_map_bounds.py accepts a float32 emulation of the kernel and rejects every
defect the emulation can switch on, on every sequence where the defect applies; the bookkeeping of the new header (binding table, exported
symbols); the host-side argument checks of both entry points through the cross-compiled library; and the checks model.attention_maps
makes before any device work (index lists, head weights, dtype, the max_bytes guard) and `map_offsets`.

The launch-log check (a default forward calls no esme_hip_attn_maps* symbol) needs the loaded library under a forward, hence a device:
it is tests/test_attn_maps_gpu.py::test_default_forward_launches_nothing_new.
"""
import ctypes
import os
import re

import pytest
import torch

import attn_map_bounds as MB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'esme_hip_attn_maps.h')
LENGTHS = (0, 1, 2, 63, 64, 65, 129, 0, 200)
H, D, L = 3, 32, 2
HEADS = [2, 0]
# mode -> (head weights?, bf16 output?, prescaled q?)
MODES = {'fp32': (False, False, False), 'bf16': (False, True, False), 'weighted': (True, False, False), 'weighted-bf16': (True, True, False),
         'q-prescaled': (False, False, True)}
_SHARED = {}


def _case(mode):
    """One batch per mode, its float64 reference and bound: computed once, shared, never modified."""
    if mode not in _SHARED:
        weighted, bf16, qp = MODES[mode]
        layers, cu, scale = MB.make_operands(LENGTHS, H, D, seed=1, qp=qp, layers=L)
        w = torch.tensor([[0.75, -1.5], [0.625, 0.5]]) if weighted else None          # (both signs; no row sums to 1)
        ref = MB.reference_maps(layers, cu, H, D, scale, HEADS, w)
        bound = MB.map_bound(layers, cu, H, D, scale, HEADS, w, out_bf16=bf16)
        _SHARED[mode] = dict(layers=layers, cu=cu, scale=scale, w=w, ref=ref, bound=bound, bf16=bf16, qp=qp)
    return _SHARED[mode]


def test_reference_is_a_softmax():
    c = _case('fp32')
    assert [tuple(r.shape) for r in c['ref']] == [(L, len(HEADS), s, s) for s in LENGTHS]
    for r in c['ref']:
        if r.numel():
            assert float((r.sum(-1) - 1).abs().max()) < 1e-12 and float(r.min()) >= 0
    w = _case('weighted')
    assert [tuple(r.shape) for r in w['ref']] == [(L, s, s) for s in LENGTHS]
    # the weighted reference is the weighted sum of the per-head reference on the same operands (same seed)
    for r, rw in zip(c['ref'], w['ref']):
        assert torch.allclose(torch.einsum('lj,ljik->lik', w['w'].double(), r), rw, rtol=0, atol=1e-12)


@pytest.mark.parametrize('mode', list(MODES))
def test_bound_accepts_the_correct_emulation(mode):
    c = _case(mode)
    got = MB.emulate_maps(c['layers'], c['cu'], H, D, c['scale'], HEADS, c['w'], out_bf16=c['bf16'])
    worst = max(MB.worst_ratio(got, c['ref'], c['bound']))
    signal = MB.signal_over_bound(c['ref'], c['bound'])
    print(f'{mode}: correct emulation: worst err / bound {worst:.3f}; smallest per-sequence peak / largest bound {signal:.0f}')
    assert worst <= 1.0
    assert signal >= 100


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('defect', MB.DEFECTS)
def test_bound_rejects_every_defect(defect, mode):
    c = _case(mode)
    weighted, bf16, qp = MODES[mode]
    got = MB.emulate_maps(c['layers'], c['cu'], H, D, c['scale'], HEADS, c['w'], out_bf16=bf16, defect=defect)
    ratios = MB.worst_ratio(got, c['ref'], c['bound'])
    T = sum(LENGTHS)
    cu = c['cu'].tolist()
    applied = 0
    for s, (S, ratio) in enumerate(zip(LENGTHS, ratios)):
        if MB.defect_applies(defect, S, T - cu[s + 1], H, L, len(HEADS), weighted, bf16, qp):      # (where it does not: its docstring)
            applied += 1
            assert ratio > 1.0, f'{mode}: the bound accepts the defect {defect!r} on the sequence of {S} rows (err / bound {ratio:.3g})'
        else:
            assert ratio <= 1.0, f'{mode}: {defect!r} is stated not to apply to the sequence of {S} rows, but changes it (err / bound {ratio:.3g})'
    print(f'{mode} {defect}: rejected on {applied} of {sum(1 for S in LENGTHS if S)} non-empty sequences; err / bound ' +
          ' '.join(f'{r:.3g}' for r in ratios))


# ------------------------------------------------------------------ the header's bookkeeping

def _declared(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r'\b(esme_hip_\w+)\s*\(([^;{}]*?)\)\s*;', text)}


def test_header_symbols_exported_and_bound():
    from esme import (_hip, _hip_attn_bwd, _hip_attn_maps, _hip_attn_pool_bwd, _hip_contact_features, _hip_contacts, _hip_gemm_wgrad,
                      _hip_optim)
    declared = set(_declared())
    assert declared == set(_hip_attn_maps.SIGNATURES) == {'esme_hip_attn_maps_workspace_bytes', 'esme_hip_attn_maps'}
    lib = ctypes.CDLL(_hip.lib_path())
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/esme_hip_attn_maps.h but not exported'
    for name, args in _declared().items():
        assert len([a for a in args.split(',') if a.strip()]) == len(_hip_attn_maps.SIGNATURES[name][1]), name
    # the other tables and headers keep their own symbols
    for other in (_hip, _hip_attn_bwd, _hip_attn_pool_bwd, _hip_contact_features, _hip_contacts, _hip_gemm_wgrad, _hip_optim):
        assert not declared & set(other.SIGNATURES), other.__name__
    for other in os.listdir(os.path.join(ROOT, 'include')):
        if other != 'esme_hip_attn_maps.h':
            assert not declared & set(_declared(os.path.join(ROOT, 'include', other))), other
            assert 'esme_hip_attn_maps' not in open(os.path.join(ROOT, 'include', other)).read(), other
    mk = open(os.path.join(ROOT, 'esm-efficient_amd', 'csrc', 'Makefile')).read()
    assert 'attn_maps.hip' in mk and 'esme_hip_attn_maps.h' in mk


def test_every_pointer_entry_point_has_a_footprint_case():
    import test_attn_maps_footprint_gpu as G
    names = [n for n, args in _declared().items() if '*' in args]
    assert names == ['esme_hip_attn_maps']
    covered = {s for c in G.CASES for s in c.symbols}
    for n in names:
        assert n in covered, f'{n}: no case in tests/test_attn_maps_footprint_gpu.py names it'
        assert re.search(rf'\b{n}\b', G.__doc__), f'{n}: missing from the docstring of tests/test_attn_maps_footprint_gpu.py'
    assert covered <= set(_declared()), covered - set(_declared())
    ids = [c.id for c in G.CASES]
    assert len(ids) == len(set(ids))


def test_workspace_formula_and_argument_checks():
    """Host-side checks need no device: the size query's stated formula, the no-ops, and every argument error, each of which returns
    before any launch."""
    from esme import _hip_attn_maps as HM
    assert HM.workspace_bytes(7, 1000, 20) == 2 * 20 * 1000 * 4
    assert HM.workspace_bytes(0, 0, 1) == 0
    for bad in ((1, 10, 0), (1, 10, -3), (-1, 10, 2), (1, -10, 2)):
        with pytest.raises(RuntimeError, match='bad sizes'):
            HM.workspace_bytes(*bad)
    lib = HM._lib()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    args = dict(q=p, k=p, ld=64, cu=p, B=1, T=8, H=2, d=32, max_len=8, scale=0.1, qp=0, heads=p, n=2, hw=None, map=p, bf16=0, off=p, slot0=0,
                ws=p, nb=1 << 20, stream=None)
    call = lambda **kw: lib.esme_hip_attn_maps(*{**args, **kw}.values())
    ARG, UNSUPPORTED = -1, -2
    # head dims
    for d in (24, 48, 8, 256):
        assert call(d=d, H=1, ld=256) == UNSUPPORTED and b'head dim' in lib.esme_hip_last_error(), d
    # sizes
    assert call(n=0) == ARG and b'bad sizes' in lib.esme_hip_last_error()
    assert call(n=-1) == ARG and call(H=0) == ARG and call(d=0) == ARG and call(B=-1) == ARG and call(T=-1) == ARG and call(slot0=-1) == ARG
    assert call(max_len=-1) == ARG and call(max_len=0) == ARG and call(T=1 << 31) == ARG and call(n=65536, nb=1 << 40) == ARG
    # null pointers
    for name in ('q', 'k', 'cu', 'heads', 'map', 'off', 'ws'):
        assert call(**{name: None}) == ARG and b'null pointer' in lib.esme_hip_last_error(), name
    # row stride and alignment
    assert call(ld=60) == ARG and call(ld=56) == ARG and b'row stride' in lib.esme_hip_last_error()
    assert call(q=p + 2) == ARG and call(k=p + 8) == ARG and call(ws=p + 4) == ARG and b'misaligned' in lib.esme_hip_last_error()
    assert call(map=p + 2) == ARG and call(map=p + 1, bf16=1) == ARG and b'misaligned' in lib.esme_hip_last_error()
    assert call(heads=p + 2) == ARG and call(hw=p + 2) == ARG and call(off=p + 4) == ARG
    # workspace one byte short (2 * n * T * 4 = 128 bytes)
    assert call(nb=127) == ARG and b'workspace too small' in lib.esme_hip_last_error()
    # the element-offset limit
    assert call(max_len=1 << 27, ld=64) == UNSUPPORTED and b'ESME_HIP_CONTACT_MAX_SEQ_ELEMS' in lib.esme_hip_last_error()
    # nothing to do: no launch
    assert call(B=0) == 0 and call(T=0) == 0


# ------------------------------------------------------------------ the Python side, no device

def test_map_offsets_with_empty_sequences():
    from esme import _hip_attn_maps as HM
    cu = torch.tensor([0, 0, 3, 3, 5, 5], dtype=torch.int32)
    S, off, total = HM.map_offsets(cu)
    assert S.tolist() == [0, 3, 0, 2, 0] and off.tolist() == [0, 0, 9, 9, 13] and total == 13
    S, off, total = HM.map_offsets(cu, 6)
    assert off.tolist() == [0, 0, 54, 54, 78] and total == 78 and off.dtype == torch.int64
    S, off, total = HM.map_offsets(torch.tensor([0], dtype=torch.int32))
    assert S.numel() == 0 and off.numel() == 0 and total == 0


def _cpu_model():
    from esme import ESM2
    return ESM2(num_layers=3, embed_dim=64, attention_heads=4)


def test_argument_checks_need_no_device():
    model = _cpu_model()
    tokens, pad = torch.zeros(12, dtype=torch.long), (torch.tensor([0, 5, 12], dtype=torch.int32), 7)
    for kw in (dict(layers=[3]), dict(layers=[-4]), dict(heads=[4]), dict(heads=[0, -5])):
        with pytest.raises(IndexError, match='out of range'):
            model.attention_maps(tokens, pad, **kw)
    for kw in (dict(layers=[0, 0]), dict(layers=[2, -1]), dict(heads=[1, 2, 1]), dict(heads=[-1, 3])):
        with pytest.raises(ValueError, match='duplicates'):
            model.attention_maps(tokens, pad, **kw)
    for hw in (torch.ones(4), torch.ones(3, 3), torch.ones(2, 4), torch.ones(3, 4, dtype=torch.long), 'sum'):
        with pytest.raises(ValueError, match='head_weights'):
            model.attention_maps(tokens, pad, head_weights=hw)
    with pytest.raises(ValueError, match='head_weights'):
        model.attention_maps(tokens, pad, layers=[0, 1], heads=[2], head_weights=torch.ones(1, 2))
    for dt in (torch.float16, torch.float64, torch.int32):
        with pytest.raises(ValueError, match='dtype'):
            model.attention_maps(tokens, pad, dtype=dt)


@pytest.mark.parametrize('kw,n_layers,n_out,item', [(dict(), 3, 4, 4), (dict(dtype=torch.bfloat16), 3, 4, 2), (dict(layers=[-1], heads=[0, 2]), 1, 2, 4),
                                                     (dict(head_weights='mean'), 3, 1, 4), (dict(layers=[0, 2], heads=[1], dtype=torch.bfloat16), 2, 1, 2)])
def test_max_bytes_refusal_states_the_formula(kw, n_layers, n_out, item):
    model = _cpu_model()
    tokens, pad = torch.zeros(12, dtype=torch.long), (torch.tensor([0, 5, 5, 12], dtype=torch.int32), 7)
    need = n_layers * n_out * (5 * 5 + 7 * 7) * item
    with pytest.raises(ValueError, match='max_bytes') as err:
        model.attention_maps(tokens, pad, max_bytes=need - 1, **kw)
    msg = str(err.value)
    assert int(re.search(r'need (\d+) bytes', msg).group(1)) == need
    for name in ('layers=', 'heads=', 'head_weights=', 'dtype='):
        assert name in msg
    # 2-D tokens: the lengths are counted from the padding
    pad_idx = model.alphabet.padding_idx
    grid = torch.full((2, 9), pad_idx, dtype=torch.long)
    grid[0, :5], grid[1, :7] = pad_idx + 3, pad_idx + 3
    with pytest.raises(ValueError, match=f'need {need} bytes'):
        model.attention_maps(grid, max_bytes=need - 1, **kw)
    # one byte more room: the guard lets the call through, and the forward then asks for a device
    with pytest.raises(Exception) as err:
        model.attention_maps(tokens, pad, max_bytes=need, **kw)
    assert 'max_bytes' not in str(err.value)


def test_refusals_by_name_need_no_device():
    model = _cpu_model()
    tokens, pad = torch.zeros(12, dtype=torch.long), (torch.tensor([0, 5, 12], dtype=torch.int32), 7)
    with pytest.raises(NotImplementedError, match='attention_maps'):
        model.graphed(tokens, pad, what='attention_maps')


def test_the_three_accumulators_share_one_layer_hook():
    from esme.attention_maps import AttentionMapAccumulator
    from esme.contacts import ContactAccumulator, ContactFeatureAccumulator
    from esme.qk_observer import QKObserver
    for cls in (ContactAccumulator, ContactFeatureAccumulator, AttentionMapAccumulator):
        assert issubclass(cls, QKObserver) and cls is not QKObserver
        assert 'layer' not in vars(cls) and cls.layer is QKObserver.layer
        assert 'launch' in vars(cls) and 'result' in vars(cls)
