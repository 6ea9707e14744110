"""Attention maps on the GPU: esme_hip_attn_maps against the float64 definition within the kernel's per-element bound
(tests/attn_map_bounds.py); head lists, slots, the weighted mode and its exact properties (determinism, batch independence, every owned
element written and nothing else); the wiring of model.attention_maps on the captured per-layer q / k for every model family; the dense
output; the end-to-end error against the oracle's fp32 forward next to the oracle's own bf16 forward; and the refusals.

End-to-end figures of the last run (profiles/attn_maps_parity.txt): see the file; the test asserts err_hip <= 2 * err_ref.
"""
import os
import tempfile

import pytest
import torch

import attn_map_bounds as MB

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LENGTHS = (0, 1, 2, 63, 64, 65, 129, 0, 200)
H = 3
F32, BF = torch.float32, torch.bfloat16


def run_maps(layer, cu, H, d, scale, heads, weights=None, dtype=F32, max_len=None):
    """One esme_hip_attn_maps call on a NaN-filled map and a 0xFF-filled workspace; returns the list of (n_out, S, S) blocks
    ((S, S) with weights)."""
    from esme import _hip, _hip_attn_maps as HM
    q, k, qp = layer
    lens = (cu[1:] - cu[:-1]).tolist()
    n_out = 1 if weights is not None else len(heads)
    S, off, total = HM.map_offsets(cu, n_out)
    out = torch.full((max(total, 1),), float('nan'), dtype=dtype, device=DEV)
    ws = torch.full((max(HM.workspace_bytes(len(lens), int(cu[-1]), len(heads)), 16),), 0xFF, dtype=torch.uint8, device=DEV)
    hl = torch.tensor(heads, dtype=torch.int32, device=DEV)
    w = None if weights is None else weights.to(device=DEV, dtype=F32).contiguous()
    with _hip.stream_scope(DEV):
        HM.attn_maps(q, k, cu, max(lens) if max_len is None else max_len, H, d, scale, hl, out, off, 0, ws, head_weights=w, q_prescaled=qp)
    torch.cuda.synchronize()
    shape = (lambda s: (s, s)) if weights is not None else (lambda s: (n_out, s, s))
    return [out[o:o + n_out * s * s].view(shape(s)) for s, o in zip(S.tolist(), off.tolist())]


def check_against_reference(got, layer, cu, H, d, scale, heads, what, weights=None, bf16=False):
    """Every element within its bound of the float64 definition; the signal stands 100 x above the largest bound."""
    w = None if weights is None else weights.reshape(1, -1)
    ref = [r[0] for r in MB.reference_maps([layer], cu, H, d, scale, heads, w)]
    bound = [b[0] for b in MB.map_bound([layer], cu, H, d, scale, heads, w, out_bf16=bf16)]
    for s, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape, (what, s, g.shape, r.shape)
        assert bool(torch.isfinite(g.float()).all()), f'{what}: sequence {s}: non-finite entries'
    worst = max(MB.worst_ratio(got, ref, bound))
    signal = MB.signal_over_bound(ref, bound)
    print(f'{what}: smallest per-sequence peak / largest bound {signal:.0f}, worst err / bound {worst:.3f}')
    # a kernel that returns zeros (or 1 / S everywhere) must not pass: every sequence's largest entry stands 100 x above the largest bound
    assert signal >= 100, (what, signal)
    assert worst <= 1.0, f'{what}: worst err / bound {worst:.3g}'
    return ref, bound


CASES = [(16, None), (32, None), (64, None), (128, None), (32, 24)]


@pytest.mark.parametrize('dtype', [F32, BF], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('qp', [False, True], ids=['scaled-in-kernel', 'q-prescaled'])
@pytest.mark.parametrize('d,logical', CASES, ids=[f'd{d}' + (f'-logical{l}' if l else '') for d, l in CASES])
def test_kernel_against_float64(d, logical, qp, dtype):
    layers, cu, scale = MB.make_operands(LENGTHS, H, d, seed=11 + d, logical_d=logical, qp=qp, device=DEV)
    assert layers[0][0].stride(0) == 3 * H * d                     # column blocks of the wider (T, 3E) buffer
    heads = list(range(H))
    got = run_maps(layers[0], cu, H, d, scale, heads, dtype=dtype)
    assert [tuple(g.shape) for g in got] == [(H, s, s) for s in LENGTHS] and got[0].dtype == dtype
    check_against_reference(got, layers[0], cu, H, d, scale, heads, f'attn_maps d{d} logical {logical} qp {qp} {dtype}', bf16=dtype == BF)


@pytest.mark.parametrize('dtype', [F32, BF], ids=['fp32', 'bf16'])
def test_head_lists_give_the_same_bits(dtype):
    d = 64
    layers, cu, scale = MB.make_operands(LENGTHS, H, d, seed=5, device=DEV)
    full = run_maps(layers[0], cu, H, d, scale, [0, 1, 2], dtype=dtype)
    for heads in ([2, 0], [1]):
        part = run_maps(layers[0], cu, H, d, scale, heads, dtype=dtype)
        for s, (p, f) in enumerate(zip(part, full)):
            assert p.shape[0] == len(heads)
            for j, h in enumerate(heads):
                assert torch.equal(p[j], f[h]), f'heads {heads}: head {h} of sequence {s} differs from the full call'


def _gapped_layout(lengths, blocks, gap):
    off, pos = [], gap
    for S in lengths:
        off.append(pos)
        pos += blocks * S * S + gap
    return torch.tensor(off, dtype=torch.int64, device=DEV), pos


def test_slot0_fills_two_layers_and_leaves_the_gaps():
    """Two calls (slot0 = 0 and n) fill the two layers' slots of one buffer whose sequences' runs are separated by a sentinel fill."""
    from esme import _hip, _hip_attn_maps as HM
    d, heads, GAP, SENT = 32, [2, 0], 41, -7.0
    layers, cu, scale = MB.make_operands(LENGTHS, H, d, seed=6, layers=2, device=DEV)
    n = len(heads)
    off, total = _gapped_layout(LENGTHS, 2 * n, GAP)
    out = torch.full((total,), SENT, dtype=F32, device=DEV)
    ws = torch.full((HM.workspace_bytes(len(LENGTHS), int(cu[-1]), n),), 0xFF, dtype=torch.uint8, device=DEV)
    hl = torch.tensor(heads, dtype=torch.int32, device=DEV)
    with _hip.stream_scope(DEV):
        for i, (q, k, qp) in enumerate(layers):
            HM.attn_maps(q, k, cu, max(LENGTHS), H, d, scale, hl, out, off, i * n, ws, q_prescaled=qp)
    torch.cuda.synchronize()
    owned = torch.zeros(total, dtype=torch.bool, device=DEV)
    alone = [run_maps(layer, cu, H, d, scale, heads) for layer in layers]
    for s, (S, o) in enumerate(zip(LENGTHS, off.tolist())):
        owned[o:o + 2 * n * S * S] = True
        block = out[o:o + 2 * n * S * S].view(2, n, S, S)
        for i in range(2):
            assert torch.equal(block[i], alone[i][s]), f'sequence {s}, layer {i}: the slots differ from a call of their own'
    assert bool((out[~owned] == SENT).all()), 'the fill between the sequences was written'
    assert not bool((out[owned] == SENT).any())


def test_weighted_mode():
    d, heads = 64, [2, 0, 1]
    layers, cu, scale = MB.make_operands(LENGTHS, H, d, seed=8, device=DEV)
    w = torch.tensor([0.75, -1.5, 0.25])
    for dtype in (F32, BF):
        got = run_maps(layers[0], cu, H, d, scale, heads, weights=w, dtype=dtype)
        assert [tuple(g.shape) for g in got] == [(s, s) for s in LENGTHS]
        check_against_reference(got, layers[0], cu, H, d, scale, heads, f'weighted {dtype}', weights=w.to(DEV), bf16=dtype == BF)
    full = run_maps(layers[0], cu, H, d, scale, heads)
    for j in range(3):                                             # a one-hot weight vector: that head's fp32 map, bit for bit
        hot = torch.zeros(3)
        hot[j] = 1.0
        got = run_maps(layers[0], cu, H, d, scale, heads, weights=hot)
        for s, (g, f) in enumerate(zip(got, full)):
            assert torch.equal(g, f[j]), f'one-hot {j}: sequence {s} differs from the head map'


def test_exact_properties():
    from esme import _hip, _hip_attn_maps as HM
    d, heads = 32, [1, 2]
    layers, cu, scale = MB.make_operands(LENGTHS, H, d, seed=3, device=DEV)
    layer = layers[0]
    got = run_maps(layer, cu, H, d, scale, heads)                 # (the map was NaN before the call, the workspace 0xFF)
    again = run_maps(layer, cu, H, d, scale, heads)
    cul = cu.tolist()
    for s, (g, g2) in enumerate(zip(got, again)):
        assert torch.equal(g, g2), f'sequence {s}: two runs differ'
        S = g.shape[-1]
        if S:
            assert not bool(torch.isnan(g).any()), f'sequence {s}: an owned element was not written'
            rows = g.double().sum(-1)
            assert float((rows - 1).abs().max()) <= S * 2.0 ** -22, f'sequence {s}: row sums off by {float((rows - 1).abs().max()):.3e}'
            a, b = cul[s], cul[s + 1]                              # the sequence alone: bit-equal to its blocks of the packed run
            one = run_maps((layer[0][a:b], layer[1][a:b], layer[2]), torch.tensor([0, b - a], dtype=torch.int32, device=DEV), H, d, scale, heads)[0]
            assert torch.equal(one, g), f'sequence {s}: alone and packed differ'
    # outside the owned blocks a NaN poison with a payload stays bit-identical; empty sequences (first, in the middle, last) own nothing
    lengths, GAP, n = (0, 5, 0, 70, 0), 29, len(heads)
    ops, cu2, scale = MB.make_operands(lengths, H, d, seed=4, device=DEV)
    off, total = _gapped_layout(lengths, n, GAP)
    poison = torch.full((total,), 0x7FC01234, dtype=torch.int32, device=DEV)
    out = poison.clone()
    ws = torch.empty(HM.workspace_bytes(len(lengths), int(cu2[-1]), n), dtype=torch.uint8, device=DEV)
    with _hip.stream_scope(DEV):
        HM.attn_maps(ops[0][0], ops[0][1], cu2, max(lengths), H, d, scale, torch.tensor(heads, dtype=torch.int32, device=DEV), out.view(F32), off, 0, ws)
    torch.cuda.synchronize()
    owned = torch.zeros(total, dtype=torch.bool, device=DEV)
    for S, o in zip(lengths, off.tolist()):
        owned[o:o + n * S * S] = True
    assert torch.equal(out[~owned], poison[~owned]), 'an element outside the owned blocks changed'
    assert not bool(torch.isnan(out.view(F32)[owned]).any())
    # only empty sequences: the buffer stays as it was
    cu0 = torch.zeros(4, dtype=torch.int32, device=DEV)
    out0 = poison[:64].clone()
    with _hip.stream_scope(DEV):
        HM.attn_maps(ops[0][0][:0], ops[0][1][:0], cu0, 1, H, d, scale, torch.tensor(heads, dtype=torch.int32, device=DEV), out0.view(F32),
                     torch.zeros(3, dtype=torch.int64, device=DEV), 0, ws)
    torch.cuda.synchronize()
    assert torch.equal(out0, poison[:64])


def test_a_row_of_scores_spanning_forty_natural_units():
    """One 300-row sequence whose query row 7 is scaled up until its scores span about 40 natural units (e^-40 = 4e-18 of the peak)."""
    d, S, row = 64, 300, 7
    g = torch.Generator().manual_seed(12)
    qkv = torch.randn(S, 3, H, d, generator=g) * 3.0 ** 0.5
    scale = d ** -0.5
    s = torch.einsum('hc,jhc->hj', qkv[row, 0].double(), qkv[:, 1].double()) * scale
    span = float((s.max(1).values - s.min(1).values).min())
    qkv[row, 0] *= 40.0 / span
    qkv = qkv.to(BF).reshape(S, 3 * H * d).to(DEV)
    layer = (qkv[:, :H * d], qkv[:, H * d:2 * H * d], False)
    s = torch.einsum('hc,jhc->hj', layer[0][row].double().view(H, d), layer[1].double().view(S, H, d)) * scale
    spans = (s.max(1).values - s.min(1).values).tolist()
    print('score spans of the scaled row, natural units: ' + ' '.join(f'{x:.1f}' for x in spans))
    assert min(spans) >= 38
    cu = torch.tensor([0, S], dtype=torch.int32, device=DEV)
    for dtype in (F32, BF):
        got = run_maps(layer, cu, H, d, scale, [0, 1, 2], dtype=dtype)
        assert bool(torch.isfinite(got[0].float()).all())
        check_against_reference(got, layer, cu, H, d, scale, [0, 1, 2], f'40-unit row {dtype}', bf16=dtype == BF)


def test_unsupported_head_dim_and_small_workspace():
    from esme import _hip_attn_maps as HM
    layers, cu, scale = MB.make_operands((5, 7), 2, 32, seed=1, device=DEV)
    q, k, _ = layers[0]
    S, off, total = HM.map_offsets(cu, 2)
    out = torch.zeros(total, dtype=F32, device=DEV)
    hl = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    ws = torch.empty(HM.workspace_bytes(2, 12, 2), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match='workspace too small'):
        HM.attn_maps(q, k, cu, 7, 2, 32, scale, hl, out, off, 0, ws[:-1])
    q24 = torch.zeros(12, 48, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match='head dim must be'):
        HM.attn_maps(q24, q24, cu, 7, 2, 24, scale, hl, out, off, 0, ws)
    assert not bool(out.any())


# ------------------------------------------------------------------ the model

MODELS = {'esm2': ('esm2', 3, 320, 20), 'esmc': ('esmc', 3, 960, 15), 'esm1b': ('esm1b', 3, 320, 20), 'esm2-padded': ('esm2', 3, 480, 20),
          'esm2-lora': ('esm2', 3, 320, 20), 'esm2-4bit': ('esm2', 3, 320, 20)}
MODEL_LENGTHS = [33, 150, 70, 2, 3]
_CACHE = {}


def _model(name):
    if name not in _CACHE:
        from esme import ESM, synthetic as syn
        kind, L, E, Hm = MODELS[name]
        with tempfile.TemporaryDirectory() as td:
            path = syn.write_checkpoint(os.path.join(td, 'm.safetensors'), f'{kind}_test', L, E, Hm, seed=23)
            model = ESM.from_pretrained(path, device=DEV, **({'quantization': '4bit'} if name == 'esm2-4bit' else {}))
        if name == 'esm2-lora':
            model.add_lora(rank=8, alpha=16, layers=('query', 'key', 'value', 'output'), adapter_names=['a'])
            g = torch.Generator().manual_seed(2)
            with torch.no_grad():
                for pname, p in model.named_parameters():
                    if '.lora_B.' in pname:                       # (zero after add_lora: give the adapters an effect on q and k)
                        p.copy_((torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5).to(p.dtype))
        _CACHE[name] = model
    return _CACHE[name]


def _batch():
    from esme import synthetic as syn
    return syn.random_tokens(MODEL_LENGTHS, seed=4).to(DEV), syn.cu_lens_of(MODEL_LENGTHS).to(DEV), max(MODEL_LENGTHS)


def _check_views(maps, n_layers, n_heads):
    assert [tuple(m.shape) for m in maps] == [(n_layers, n_heads, s, s) for s in MODEL_LENGTHS]
    base = maps[0].untyped_storage().data_ptr()
    assert all(m.untyped_storage().data_ptr() == base for m in maps), 'the views do not share one storage'
    offs = [m.storage_offset() for m in maps]
    assert offs == sorted(offs) and offs[0] == 0                   # batch order


@pytest.mark.parametrize('name', list(MODELS))
def test_wiring_on_captured_qk(name):
    model = _model(name)
    kind, L, E, Hm = MODELS[name]
    tokens, cu, ml = _batch()
    d, scale = model.head_pad, (E // Hm) ** -0.5
    for kw, lsel, hsel in ((dict(layers=[0, -1], heads=None), [0, L - 1], list(range(Hm))), (dict(layers=None, heads=[1]), list(range(L)), [1])):
        maps = model.attention_maps(tokens, (cu, ml), _keep_qk=True, **kw)
        torch.cuda.synchronize()
        qk = model._contact_qk
        assert [i for i, *_ in qk] == list(range(L))
        assert qk[0][1].shape == (tokens.numel(), Hm * d)
        _check_views(maps, len(lsel), len(hsel))
        assert maps[0].dtype == F32
        layers = [(qk[l][1], qk[l][2], qk[l][3]) for l in lsel]
        ref = MB.reference_maps(layers, cu, Hm, d, scale, hsel)
        bound = MB.map_bound(layers, cu, Hm, d, scale, hsel)
        worst = max(MB.worst_ratio(maps, ref, bound))
        signal = MB.signal_over_bound(ref, bound)
        print(f'attention_maps {name} {kw}: smallest per-sequence peak / largest bound {signal:.0f}, worst err / bound {worst:.3f}')
        assert signal >= 100 and worst <= 1.0, (name, kw, signal, worst)


def test_weights_dtype_and_lora_names_through_the_model():
    model = _model('esm2')
    kind, L, E, Hm = MODELS['esm2']
    tokens, cu, ml = _batch()
    full = model.attention_maps(tokens, (cu, ml), layers=[-1, 0], heads=[3, 7, 0])
    mean = model.attention_maps(tokens, (cu, ml), layers=[-1, 0], heads=[3, 7, 0], head_weights='mean')
    w = torch.tensor([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])
    hot = model.attention_maps(tokens, (cu, ml), layers=[-1, 0], heads=[3, 7, 0], head_weights=w)
    half = model.attention_maps(tokens, (cu, ml), layers=[-1, 0], heads=[3, 7, 0], dtype=BF)
    for f, m, h, b, S in zip(full, mean, hot, half, MODEL_LENGTHS):
        assert m.shape == h.shape == (2, S, S) and b.dtype == BF
        assert torch.equal(h[0], f[0, 1]) and torch.equal(h[1], f[1, 0])                   # one-hot rows pick a head, bit for bit
        third = torch.tensor(1.0 / 3.0, dtype=F32, device=DEV)
        acc = torch.zeros_like(f[:, 0])
        for j in range(3):
            acc = torch.addcmul(acc, third, f[:, j])                                       # (not fused: within one rounding per step)
        assert torch.allclose(m, acc, rtol=0, atol=4 * 2.0 ** -24)
        assert torch.equal(b, f.to(BF))                                                    # the bf16 map is the RNE image of the fp32 map
    lora = _model('esm2-lora')
    a = lora.attention_maps(tokens, (cu, ml), layers=[-1], heads=[0], lora_names=['a'])
    base = model.attention_maps(tokens, (cu, ml), layers=[-1], heads=[0])
    assert not torch.equal(a[1], base[1])                          # the adapters reach q and k


def test_dense_output_places_the_blocks():
    model = _model('esm2')
    tokens, cu, ml = _batch()
    for kw, lead in ((dict(layers=[0, -1], heads=[4, 2]), (2, 2)), (dict(layers=[1], head_weights='mean'), (1,))):
        packed = model.attention_maps(tokens, (cu, ml), **kw)
        dense = model.attention_maps(tokens, (cu, ml), pad_output=True, **kw)
        assert dense.shape == (len(MODEL_LENGTHS), *lead, ml, ml) and dense.dtype == F32
        pad = model.alphabet.padding_idx
        grid = torch.full((len(MODEL_LENGTHS), ml + 3), pad, dtype=tokens.dtype, device=DEV)      # 2-D tokens, wider than the longest protein
        cul = cu.tolist()
        for s, n in enumerate(MODEL_LENGTHS):
            grid[s, :n] = tokens[cul[s]:cul[s + 1]]
        dense2 = model.attention_maps(grid, **kw)
        assert dense2.shape == (len(MODEL_LENGTHS), *lead, ml + 3, ml + 3)
        for s, p in enumerate(packed):
            n = p.shape[-1]
            for dn in (dense, dense2):
                assert torch.equal(dn[s, ..., :n, :n], p)
                rest = dn[s].clone()
                rest[..., :n, :n] = 0
                assert not bool(rest.any()), f'sequence {s}: values outside its block'


def _oracle_maps(kind, L, E, Hm, tokens, cu, ml, lsel, hsel, dtype):
    """float64 maps from the q_rot / k_rot taps of the oracle's forward in `dtype`."""
    from esme import synthetic as syn
    from oracle import esm_oracle as O
    weights = syn.synthetic_state_dict(kind, L, E, 23)
    taps = []
    O.forward_representation(weights, Hm, tokens.cpu(), cu.cpu(), ml, dtype, taps=taps)
    assert len(taps) == L
    d = E // Hm
    layers = [(taps[l]['q_rot'], taps[l]['k_rot'], False) for l in lsel]
    return MB.reference_maps(layers, cu.cpu(), Hm, d, d ** -0.5, hsel)


@pytest.mark.parametrize('name', ['esm2', 'esmc'])
def test_end_to_end_against_the_oracle(name):
    model = _model(name)
    kind, L, E, Hm = MODELS[name]
    tokens, cu, ml = _batch()
    lsel, hsel = list(range(L)), list(range(Hm))
    ours = model.attention_maps(tokens, (cu, ml))
    ref32 = _oracle_maps(kind, L, E, Hm, tokens, cu, ml, lsel, hsel, torch.float32)
    ref16 = _oracle_maps(kind, L, E, Hm, tokens, cu, ml, lsel, hsel, torch.bfloat16)
    err_hip = max(float((o.double().cpu() - r).abs().max()) for o, r in zip(ours, ref32) if r.numel())
    err_ref = max(float((b - r).abs().max()) for b, r in zip(ref16, ref32) if r.numel())
    line = f'{name}: err_hip = max |ours - oracle fp32| = {err_hip:.3e}   err_ref = max |oracle bf16 - oracle fp32| = {err_ref:.3e}   ratio {err_hip / err_ref:.2f}'
    print(line)
    if os.environ.get('ESME_ATTN_MAPS_PARITY_OUT'):              # (how profiles/attn_maps_parity.txt is written)
        with open(os.environ['ESME_ATTN_MAPS_PARITY_OUT'], 'a') as fh:
            fh.write(line + '\n')
    assert err_hip <= 2 * err_ref, line


def test_refusals():
    model = _model('esm2')
    tokens, cu, ml = _batch()
    try:
        for mode in ('half', 'exact', 'high'):
            model.set_precision(mode)
            with pytest.raises(NotImplementedError, match=f"attention_maps.*precision '{mode}'"):
                model.attention_maps(tokens, (cu, ml))
    finally:
        model.set_precision('fast')
    with pytest.raises(NotImplementedError, match='attention_maps'):
        model.graphed(tokens, (cu, ml), what='attention_maps')
    with pytest.raises(ValueError, match='max_bytes'):
        model.attention_maps(tokens, (cu, ml), max_bytes=1 << 20)


def test_default_forward_launches_nothing_new(monkeypatch):
    """A forward without a map request calls no esme_hip_attn_maps* symbol (and a map request does: the recorder sees it)."""
    from esme import _hip
    model = _model('esm2')
    tokens, cu, ml = _batch()
    lib, called = _hip.load(), []

    class Recorder:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if not name.startswith('esme_hip_') or not callable(fn):
                return fn

            def wrapped(*a):
                called.append(name)
                return fn(*a)
            return wrapped
    model.attention_maps(tokens, (cu, ml), layers=[0], heads=[0])                          # (types the symbols on the handle)
    monkeypatch.setattr(_hip, '_lib', Recorder())
    model(tokens, (cu, ml))
    model.forward_representation(tokens, (cu, ml), layers=[1])
    model.predict_log_prob(tokens, (cu, ml))
    assert called and not [n for n in called if n.startswith('esme_hip_attn_maps')], sorted(set(called))
    del called[:]
    model.attention_maps(tokens, (cu, ml), layers=[0, 2], heads=[0])
    monkeypatch.undo()
    assert called.count('esme_hip_attn_maps') == 2 and called.count('esme_hip_attn_maps_workspace_bytes') == 1


def test_statistics_are_the_contact_kernels_bit_for_bit():
    """attn_map_stats_kernel and contact_stats_kernel are one pass (softmax_row_stats of csrc/score_tiles.h): on the same (q, k, cu_lens)
    the row maxima m and row sums l that esme_hip_attn_maps leaves in its workspace (ws, ws + n_heads * T) for the head list [0, 1] have
    the bits of those esme_hip_contact_layer leaves (ws, ws + H * T) without a trim."""
    from esme import _hip, _hip_attn_maps as HM, _hip_contacts as HC
    d, heads, lengths = 32, 2, (2, 3, 65)
    layers, cu, scale = MB.make_operands(lengths, heads, d, seed=23, device=DEV)
    q, k, qp = layers[0]
    B, T = len(lengths), int(cu[-1])
    ws_m = torch.full((HM.workspace_bytes(B, T, heads),), 0xFF, dtype=torch.uint8, device=DEV)
    ws_c = torch.full((HC.workspace_bytes(B, T, heads),), 0xFF, dtype=torch.uint8, device=DEV)
    _, off_m, total_m = HM.map_offsets(cu, heads)
    _, off_c, total_c = HC.map_offsets(cu, 0, 0)
    out_m = torch.empty(total_m, dtype=F32, device=DEV)
    out_c = torch.empty(total_c, dtype=F32, device=DEV)
    with _hip.stream_scope(DEV):
        HM.attn_maps(q, k, cu, max(lengths), heads, d, scale, torch.tensor([0, 1], dtype=torch.int32, device=DEV), out_m, off_m, 0, ws_m,
                     q_prescaled=qp)
        HC.contact_layer(q, k, cu, max(lengths), heads, d, scale, torch.ones(heads, dtype=F32, device=DEV), 0.0, True, out_c, off_c, ws_c,
                         q_prescaled=qp, trim_front=0, trim_back=0)
    torch.cuda.synchronize()
    stats_m = ws_m.view(F32)[:2 * heads * T].view(2, heads, T)
    stats_c = ws_c.view(F32)[:2 * heads * T].view(2, heads, T)
    assert bool(torch.isfinite(stats_m).all()) and bool((stats_m[1] >= 1.0).all())     # every row written; l holds the maximum's exp2(0)
    assert torch.equal(stats_m.view(torch.int32), stats_c.view(torch.int32))
