"""Contact prediction on the GPU: esme_hip_contact_layer against the float64 definition within the kernel's per-element bound
(tests/contact_bounds.py), its exact properties (symmetry, batch independence, determinism), the wiring of model.predict_contacts on the
captured per-layer q / k, the end-to-end error against the oracle's fp32 forward next to the oracle's own bf16 forward, and the refusals.

End-to-end figures of the last run (profiles/contacts_parity.txt): see the file; the test asserts err_hip <= 2 * err_ref.
"""
import os
import tempfile

import pytest
import torch

import contact_bounds as CB

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LENGTHS = (0, 1, 2, 3, 18, 66, 67, 130, 195)          # n = 0, 0, 0, 1, 16, 64, 65, 128, 193
BIAS = -0.75


def _weights(L, H, seed=5):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(L, H, generator=g)
    assert bool((w > 0).any()) and bool((w < 0).any())
    return w.to(DEV)


def run_kernel(layers, cu, H, d, scale, w, bias, f=1, e=1, max_len=None):
    """One esme_hip_contact_layer call per layer on a NaN-filled map and workspace; returns the list of (n, n) maps."""
    from esme import _hip, _hip_contacts as HC
    lens = (cu[1:] - cu[:-1]).tolist()
    max_len = max(lens) if max_len is None else max_len
    n, off, total = HC.map_offsets(cu, f, e)
    out = torch.full((total,), float('nan'), dtype=torch.float32, device=DEV)
    ws = torch.full((max(HC.workspace_bytes(len(lens), int(cu[-1]), H), 16),), 0xFF, dtype=torch.uint8, device=DEV)
    with _hip.stream_scope(DEV):
        for l, (q, k, qp) in enumerate(layers):
            if total:
                HC.contact_layer(q, k, cu, max_len, H, d, scale, w[l].contiguous(), bias, l == 0, out, off, ws, q_prescaled=qp, trim_front=f, trim_back=e)
    torch.cuda.synchronize()
    return [out[o:o + m * m].view(m, m) for m, o in zip(n.tolist(), off.tolist())]


def check_against_reference(got, layers, cu, H, d, scale, w, bias, what, f=1, e=1):
    ref = CB.reference_contacts(layers, cu, H, d, scale, w, bias, f, e)
    bound = CB.contact_bound(layers, cu, H, d, scale, w, bias, f, e)
    top = max(float(b.max()) for b in bound if b.numel())
    signal = max(float((r - bias).abs().max()) for r in ref if r.numel())
    worst = 0.0
    for s, (g, r, b) in enumerate(zip(got, ref, bound)):
        assert g.shape == r.shape
        if not g.numel():
            continue
        assert bool(torch.isfinite(g).all()), f'{what}: sequence {s}: non-finite logits'
        ratio = (g.double() - r).abs() / b
        worst = max(worst, float(ratio.max()))
    print(f'{what}: max |logit - bias| {signal:.3e}, largest bound {top:.3e}, worst err / bound {worst:.3f}')
    # a kernel that returns the bias everywhere must not pass: the signal stands 100 x above the largest bound
    assert signal >= 100 * top, (what, signal, top)
    assert worst <= 1.0, f'{what}: worst err / bound {worst:.3g}'
    return ref, bound


CASES = [(20, 16, None), (5, 32, None), (3, 64, None), (2, 128, None), (4, 32, 24)]


@pytest.mark.parametrize('qp', [False, True], ids=['scaled-in-kernel', 'q-prescaled'])
@pytest.mark.parametrize('H,d,logical', CASES, ids=[f'H{h}-d{d}' + (f'-logical{l}' if l else '') for h, d, l in CASES])
def test_kernel_against_float64(H, d, logical, qp):
    layers, cu, scale = CB.make_operands(LENGTHS, H, d, seed=11 + d, logical_d=logical, qp=qp, device=DEV)
    assert layers[0][0].stride(0) == 3 * H * d                     # column views of the fused (T, 3E) buffer
    w = _weights(2, H)
    got = run_kernel(layers, cu, H, d, scale, w, BIAS)
    assert [g.shape[0] for g in got] == [0, 0, 0, 1, 16, 64, 65, 128, 193]
    check_against_reference(got, layers, cu, H, d, scale, w, BIAS, f'contact_layer H{H} d{d} logical {logical} qp {qp}')


def test_exact_properties():
    H, d = 5, 32
    layers, cu, scale = CB.make_operands(LENGTHS, H, d, seed=3, device=DEV)
    w = _weights(2, H)
    got = run_kernel(layers, cu, H, d, scale, w, BIAS)
    again = run_kernel(layers, cu, H, d, scale, w, BIAS)
    cul = cu.tolist()
    for s, (g, g2) in enumerate(zip(got, again)):
        assert torch.equal(g, g.T), f'sequence {s}: the map is not exactly symmetric'
        assert torch.equal(g, g2), f'sequence {s}: two runs differ'
        if g.numel():                                              # the sequence alone: bit-equal to its block of the packed run
            a, b = cul[s], cul[s + 1]
            alone = [(q[a:b], k[a:b], qp) for q, k, qp in layers]
            one = run_kernel(alone, torch.tensor([0, b - a], dtype=torch.int32, device=DEV), H, d, scale, w, BIAS)[0]
            assert torch.equal(one, g), f'sequence {s}: alone and packed differ'


def test_unsupported_head_dim_and_small_workspace():
    from esme import _hip_contacts as HC
    layers, cu, scale = CB.make_operands((5, 7), 2, 32, seed=1, layers=1, device=DEV)
    q, k, _ = layers[0]
    n, off, total = HC.map_offsets(cu, 1, 1)
    out = torch.zeros(total, dtype=torch.float32, device=DEV)
    w = torch.ones(2, device=DEV)
    ws = torch.empty(HC.workspace_bytes(2, 12, 2), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match='workspace too small'):
        HC.contact_layer(q, k, cu, 7, 2, 32, scale, w, 0.0, True, out, off, ws[:-16])
    q48 = torch.zeros(12, 96, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match='head dim must be'):
        HC.contact_layer(q48, q48, cu, 7, 2, 48, scale, w, 0.0, True, out, off, ws)


# ------------------------------------------------------------------ the model

MODELS = {'esm2': ('esm2', 2, 320, 20), 'esmc': ('esmc', 2, 960, 15), 'esm2-padded': ('esm2', 2, 480, 20), 'esm2-lora': ('esm2', 2, 320, 20)}
MODEL_LENGTHS = [33, 150, 70, 2, 3]
_CACHE = {}


def _model(name):
    if name not in _CACHE:
        from esme import ESM, ContactHead, synthetic as syn
        kind, L, E, H = MODELS[name]
        with tempfile.TemporaryDirectory() as td:
            path = syn.write_checkpoint(os.path.join(td, 'm.safetensors'), f'{kind}_test', L, E, H, seed=23)
            model = ESM.from_pretrained(path, device=DEV)
        if name == 'esm2-lora':
            model.add_lora(rank=8, alpha=16, layers=('query', 'key', 'value', 'output'), adapter_names=['a'])
            g = torch.Generator().manual_seed(2)
            with torch.no_grad():
                for pname, p in model.named_parameters():
                    if '.lora_B.' in pname:                       # (zero after add_lora: give the adapters an effect on q and k)
                        p.copy_((torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5).to(p.dtype))
        head = ContactHead(L, H)
        g = torch.Generator().manual_seed(9)
        head.regression.weight.data.copy_(torch.randn(1, L * H, generator=g))
        head.regression.bias.data.fill_(BIAS)
        model.set_contact_head(head)
        _CACHE[name] = model
    return _CACHE[name]


def _batch():
    from esme import synthetic as syn
    return syn.random_tokens(MODEL_LENGTHS, seed=4).to(DEV), syn.cu_lens_of(MODEL_LENGTHS).to(DEV), max(MODEL_LENGTHS)


@pytest.mark.parametrize('name', list(MODELS))
def test_wiring_on_captured_qk(name):
    model = _model(name)
    kind, L, E, H = MODELS[name]
    tokens, cu, ml = _batch()
    got = model.predict_contacts(tokens, (cu, ml), logits=True, _keep_qk=True)
    torch.cuda.synchronize()
    qk = model._contact_qk
    assert [i for i, *_ in qk] == list(range(L))
    layers = [(q, k, qp) for _, q, k, qp in qk]
    d = model.head_pad
    assert layers[0][0].shape == (tokens.numel(), H * d)
    w = model.contact_head.regression.weight.detach().reshape(L, H)
    assert [g.shape[0] for g in got] == [max(n - 2, 0) for n in MODEL_LENGTHS]
    check_against_reference(got, layers, cu, H, d, (E // H) ** -0.5, w, BIAS, f'predict_contacts {name}')
    prob = model.predict_contacts(tokens, (cu, ml))
    for p, g in zip(prob, got):
        assert torch.equal(p, torch.sigmoid(g))


def test_padded_output_places_the_blocks():
    from esme import synthetic as syn
    model = _model('esm2')
    tokens, cu, ml = _batch()
    packed = model.predict_contacts(tokens, (cu, ml), logits=True)
    dense = model.predict_contacts(tokens, (cu, ml), pad_output=True, logits=True)
    assert dense.shape == (len(MODEL_LENGTHS), ml - 2, ml - 2) and dense.dtype == torch.float32
    pad = model.alphabet.padding_idx
    grid = torch.full((len(MODEL_LENGTHS), ml + 3), pad, dtype=tokens.dtype, device=DEV)      # 2-D tokens, wider than the longest protein
    cul = cu.tolist()
    for s, n in enumerate(MODEL_LENGTHS):
        grid[s, :n] = tokens[cul[s]:cul[s + 1]]
    dense2 = model.predict_contacts(grid, logits=True)
    assert dense2.shape == (len(MODEL_LENGTHS), ml + 1, ml + 1)
    for s, p in enumerate(packed):
        n = p.shape[0]
        for dn in (dense, dense2):
            assert torch.equal(dn[s, :n, :n], p)
            rest = dn[s].clone()
            rest[:n, :n] = 0
            assert not bool(rest.any()), f'sequence {s}: values outside its block'


def _oracle_logits(kind, L, E, H, tokens, cu, ml, w, dtype):
    """Contact logits in float64 from the q_rot / k_rot taps of the oracle's forward in `dtype`."""
    from esme import synthetic as syn
    from oracle import esm_oracle as O
    weights = syn.synthetic_state_dict(kind, L, E, 23)
    taps = []
    O.forward_representation(weights, H, tokens.cpu(), cu.cpu(), ml, dtype, taps=taps)
    d = E // H
    layers = [(t['q_rot'], t['k_rot'], False) for t in taps]
    assert len(layers) == L
    return CB.reference_contacts(layers, cu.cpu(), H, d, d ** -0.5, w.cpu(), BIAS)


@pytest.mark.parametrize('name', ['esm2', 'esmc'])
def test_end_to_end_against_the_oracle(name):
    model = _model(name)
    kind, L, E, H = MODELS[name]
    tokens, cu, ml = _batch()
    ours = model.predict_contacts(tokens, (cu, ml), logits=True)
    w = model.contact_head.regression.weight.detach().reshape(L, H)
    ref32 = _oracle_logits(kind, L, E, H, tokens, cu, ml, w, torch.float32)
    ref16 = _oracle_logits(kind, L, E, H, tokens, cu, ml, w, torch.bfloat16)
    err_hip = max(float((o.double().cpu() - r).abs().max()) for o, r in zip(ours, ref32) if r.numel())
    err_ref = max(float((b - r).abs().max()) for b, r in zip(ref16, ref32) if r.numel())
    line = f'{name}: err_hip = max |ours - oracle fp32| = {err_hip:.3e}   err_ref = max |oracle bf16 - oracle fp32| = {err_ref:.3e}   ratio {err_hip / err_ref:.2f}'
    print(line)
    if os.environ.get('ESME_CONTACTS_PARITY_OUT'):               # (how profiles/contacts_parity.txt is written)
        with open(os.environ['ESME_CONTACTS_PARITY_OUT'], 'a') as fh:
            fh.write(line + '\n')
    assert err_hip <= 2 * err_ref, line


def test_refusals():
    model = _model('esm2')
    tokens, cu, ml = _batch()
    try:
        for mode in ('half', 'exact', 'high'):
            model.set_precision(mode)
            with pytest.raises(NotImplementedError, match='precision'):
                model.predict_contacts(tokens, (cu, ml))
    finally:
        model.set_precision('fast')
    with pytest.raises(NotImplementedError, match='predict_contacts'):
        model.graphed(tokens, (cu, ml), what='predict_contacts')
    head, model.contact_head = model.contact_head, None
    try:
        with pytest.raises(RuntimeError, match='contact head'):
            model.predict_contacts(tokens, (cu, ml))
    finally:
        model.contact_head = head
