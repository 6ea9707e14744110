"""Contact-regression features on the GPU: esme_hip_contact_features against the float64 definition within the gather kernel's
per-element bound (tests/contact_feature_bounds.py), its exact properties (pair symmetry, independence of the batch, of the list order and
of P, determinism, untouched columns, NaN rows for out-of-range pairs), the wiring of model.contact_features on the captured per-layer
q / k next to predict_contacts, LoRA adapters, fit_contact_head end to end, the refusals, and the default forward's unchanged launch list.
"""
import os
import tempfile

import pytest
import torch

import contact_bounds as CB
import contact_feature_bounds as FB

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LENGTHS = (0, 1, 2, 3, 18, 66, 67, 130, 195, 0)       # n = 0, 0, 0, 1, 16, 64, 65, 128, 193, 0
SENTINEL = -12345.0


def run_kernel(layers, cu, H, d, scale, pairs, f=1, e=1, max_len=None, extra=(0, 0), fill=SENTINEL):
    """One esme_hip_contact_features call per layer (col0 = extra[0] + l * H) into a `fill`-filled (P, extra[0] + L * H + extra[1]) matrix
    with a 0xFF-filled workspace; returns the whole matrix."""
    from esme import _hip, _hip_contact_features as HF
    lens = (cu[1:] - cu[:-1]).tolist()
    max_len = max(lens) if max_len is None else max_len
    L = len(layers)
    feat = torch.full((pairs.shape[0], extra[0] + L * H + extra[1]), fill, dtype=torch.float32, device=DEV)
    ws = torch.full((max(HF.workspace_bytes(len(lens), int(cu[-1]), H), 16),), 0xFF, dtype=torch.uint8, device=DEV)
    with _hip.stream_scope(DEV):
        for l, (q, k, qp) in enumerate(layers):
            HF.contact_features(q, k, cu, max_len, H, d, scale, pairs, feat, extra[0] + l * H, ws, q_prescaled=qp, trim_front=f, trim_back=e)
    torch.cuda.synchronize()
    return feat


def check_against_reference(got, layers, cu, H, d, scale, pairs, what, f=1, e=1):
    ref = FB.reference_features(layers, cu, H, d, scale, pairs, f, e)
    bound = FB.feature_bound(layers, cu, H, d, scale, pairs, f, e)
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), f'{what}: non-finite features'
    worst = float(((got.double() - ref).abs() / bound).max())
    signal, top = float(ref.abs().max()), float(bound.max())
    print(f'{what}: max |N| {signal:.3e}, largest bound {top:.3e}, worst err / bound {worst:.3f}')
    assert signal >= 100 * top, (what, signal, top)              # a kernel that returns zeros must not pass
    assert worst <= 1.0, f'{what}: worst err / bound {worst:.3g}'
    return ref, bound


CASES = [(20, 16, None), (5, 32, None), (3, 32, 24), (3, 64, None), (2, 128, None)]


@pytest.mark.parametrize('qp', [False, True], ids=['scaled-in-kernel', 'q-prescaled'])
@pytest.mark.parametrize('H,d,logical', CASES, ids=[f'H{h}-d{d}' + (f'-logical{l}' if l else '') for h, d, l in CASES])
def test_kernel_against_float64(H, d, logical, qp):
    layers, cu, scale = FB.make_operands(LENGTHS, H, d, seed=11 + d, logical_d=logical, qp=qp, device=DEV)
    assert layers[0][0].stride(0) == 3 * H * d                     # column views of the fused (T, 3E) buffer
    pairs = FB.make_pairs(LENGTHS, seed=d).to(DEV)
    got = run_kernel(layers, cu, H, d, scale, pairs)               # two layers into one matrix through col0
    check_against_reference(got, layers, cu, H, d, scale, pairs, f'contact_features H{H} d{d} logical {logical} qp {qp}')


def test_kernel_against_float64_untrimmed():
    H, d = 3, 64
    layers, cu, scale = FB.make_operands(LENGTHS, H, d, seed=5, device=DEV)
    pairs = FB.make_pairs(LENGTHS, 0, 0, seed=6).to(DEV)
    assert int(pairs[:, 1:].max()) == 194                          # the last row of the longest sequence
    got = run_kernel(layers, cu, H, d, scale, pairs, f=0, e=0)
    check_against_reference(got, layers, cu, H, d, scale, pairs, 'contact_features trims (0, 0)', f=0, e=0)


def test_exact_properties():
    H, d = 5, 32
    layers, cu, scale = FB.make_operands(LENGTHS, H, d, seed=3, device=DEV)
    pairs = FB.make_pairs(LENGTHS, seed=4).to(DEV)
    P = pairs.shape[0]
    got = run_kernel(layers, cu, H, d, scale, pairs, extra=(3, 2))
    assert bool((got[:, :3] == SENTINEL).all()) and bool((got[:, -2:] == SENTINEL).all()), 'columns outside col0 .. col0 + H - 1 were written'
    X = got[:, 3:-2]
    assert bool(torch.isfinite(X).all())
    assert torch.equal(X, run_kernel(layers, cu, H, d, scale, pairs)), 'the features depend on col0 / ld_feat'
    assert torch.equal(got, run_kernel(layers, cu, H, d, scale, pairs, extra=(3, 2))), 'two runs differ'
    # (i, j) and (j, i); duplicates
    swapped = pairs[:, [0, 2, 1]].contiguous()
    assert torch.equal(run_kernel(layers, cu, H, d, scale, swapped), X), '(i, j) and (j, i) differ'
    rows = {}
    for p, r in enumerate(pairs.tolist()):
        rows.setdefault(tuple(r), []).append(p)
    dup = [v for v in rows.values() if len(v) > 1]
    assert dup and all(torch.equal(X[v[0]], X[p]) for v in dup for p in v[1:])
    # list order and P: a permutation, and a short prefix
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(1)).to(DEV)
    assert torch.equal(run_kernel(layers, cu, H, d, scale, pairs[perm].contiguous()), X[perm]), 'the rows depend on the list order'
    assert torch.equal(run_kernel(layers, cu, H, d, scale, pairs[:7].contiguous()), X[:7]), 'the rows depend on P'
    # every sequence alone: bit-equal to its rows of the packed run
    cul = cu.tolist()
    for s in pairs[:, 0].unique().tolist():
        a, b = cul[s], cul[s + 1]
        sel = (pairs[:, 0] == s).nonzero().reshape(-1)
        own = pairs[sel].clone()
        own[:, 0] = 0
        alone = [(q[a:b], k[a:b], qp) for q, k, qp in layers]
        one = run_kernel(alone, torch.tensor([0, b - a], dtype=torch.int32, device=DEV), H, d, scale, own.contiguous())
        assert torch.equal(one, X[sel]), f'sequence {s}: alone and packed differ'
    # P = 0 writes nothing
    from esme import _hip_contact_features as HF
    lib = HF._lib()
    q, k, qp = layers[0]
    feat = torch.full((4, H), SENTINEL, device=DEV)
    ws = torch.empty(HF.workspace_bytes(len(LENGTHS), int(cu[-1]), H), dtype=torch.uint8, device=DEV)
    rc = lib.esme_hip_contact_features(q.data_ptr(), k.data_ptr(), q.stride(0), cu.data_ptr(), len(LENGTHS), int(cu[-1]), H, d, max(LENGTHS), scale, 0, 1, 1,
                                       pairs.data_ptr(), 0, feat.data_ptr(), H, 0, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and bool((feat == SENTINEL).all())


def test_out_of_range_pairs_give_nan_rows_and_errors_launch_nothing():
    from esme import _hip_contact_features as HF
    from esme.contacts import check_pairs
    H, d = 3, 64
    lengths = (18, 0, 67)                                          # n = 16, 0, 65
    layers, cu, scale = FB.make_operands(lengths, H, d, seed=8, layers=1, device=DEV)
    good = torch.tensor([[0, 0, 15], [2, 64, 3], [2, 10, 10], [0, 7, 2]], dtype=torch.int32)
    bad = torch.tensor([[0, 0, 16], [0, 16, 0], [1, 0, 0], [3, 0, 0], [-1, 0, 0], [2, -1, 4], [2, 4, -1], [2, 65, 65], [2 ** 31 - 1, 0, 0],
                        [0, 2 ** 31 - 1, 0], [-2 ** 31, -2 ** 31, -2 ** 31], [2, 0, 66]], dtype=torch.int32)
    mixed = torch.stack([r for pair in zip(bad, good.repeat(3, 1)) for r in pair]).contiguous().to(DEV)      # bad, good, bad, good, ...
    got = run_kernel(layers, cu, H, d, scale, mixed, extra=(1, 1))
    assert bool((got[:, 0] == SENTINEL).all()) and bool((got[:, -1] == SENTINEL).all())
    X = got[:, 1:-1]
    assert bool(torch.isnan(X[0::2]).all()), 'an out-of-range pair did not give a NaN row'
    clean = run_kernel(layers, cu, H, d, scale, good.to(DEV))
    assert bool(torch.isfinite(clean).all()) and torch.equal(X[1::2], clean.repeat(3, 1)), 'an out-of-range pair disturbed its neighbours'
    # Python refuses the same list
    with pytest.raises(ValueError, match='out of range'):
        check_pairs(mixed, [16, 0, 65], DEV)
    assert torch.equal(check_pairs(good, [16, 0, 65], DEV), good.to(DEV))
    # an unsupported head dim and a short workspace are refused before any launch: the return code, and nothing written
    lib = HF._lib()
    q, k, _ = layers[0]
    T, B = int(cu[-1]), len(lengths)
    pairs = good.to(DEV)
    feat = torch.full((4, H), SENTINEL, device=DEV)
    need = HF.workspace_bytes(B, T, H)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda dd, nbytes: lib.esme_hip_contact_features(q.data_ptr(), k.data_ptr(), q.stride(0), cu.data_ptr(), B, T, H, dd, max(lengths), scale, 0, 1, 1,
                                                            pairs.data_ptr(), 4, feat.data_ptr(), H, 0, ws.data_ptr(), nbytes, stream)
    assert call(48, need) == -2 and b'head dim' in lib.esme_hip_last_error()          # ESME_ERR_UNSUPPORTED
    assert call(d, need - 16) == -1 and b'workspace too small' in lib.esme_hip_last_error()      # ESME_ERR_ARG
    torch.cuda.synchronize()
    assert bool((feat == SENTINEL).all())
    assert call(d, need) == 0
    torch.cuda.synchronize()
    assert torch.equal(feat, clean)


# ------------------------------------------------------------------ the model

MODELS = {'esm2': ('esm2', 2, 320, 20), 'esmc': ('esmc', 2, 960, 15), 'esm1b': ('esm1b', 2, 320, 20), 'esm2-padded': ('esm2', 2, 480, 20),
          'esm2-lora': ('esm2', 2, 320, 20)}
MODEL_LENGTHS = [33, 150, 70, 2, 3]
BIAS = -0.75
_CACHE = {}


def _model(name):
    if name not in _CACHE:
        from esme import ESM, synthetic as syn
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
        _CACHE[name] = model
    return _CACHE[name]


def _random_head(L, H, seed=9):
    from esme import ContactHead
    head = ContactHead(L, H)
    head.regression.weight.data.copy_(torch.randn(1, L * H, generator=torch.Generator().manual_seed(seed)))
    head.regression.bias.data.fill_(BIAS)
    return head


def _batch():
    from esme import synthetic as syn
    return syn.random_tokens(MODEL_LENGTHS, seed=4).to(DEV), syn.cu_lens_of(MODEL_LENGTHS).to(DEV), max(MODEL_LENGTHS)


def _captured(model, L):
    qk = model._contact_qk
    assert [i for i, *_ in qk] == list(range(L))
    return [(q, k, qp) for _, q, k, qp in qk]


@pytest.mark.parametrize('name', ['esm2', 'esmc', 'esm1b', 'esm2-padded'])
def test_wiring_on_captured_qk(name):
    model = _model(name)
    kind, L, E, H = MODELS[name]
    tokens, cu, ml = _batch()
    d, scale = model.head_pad, (E // H) ** -0.5
    pairs = FB.make_pairs(MODEL_LENGTHS, seed=1, random_pairs=60).to(DEV)
    assert model.contact_head is None                              # contact_features needs no head
    X, back = model.contact_features(tokens, (cu, ml), pairs=pairs, _keep_qk=True)
    torch.cuda.synchronize()
    layers = _captured(model, L)
    assert layers[0][0].shape == (tokens.numel(), H * d)
    assert X.dtype == torch.float32 and X.shape == (pairs.shape[0], L * H) and back.dtype == torch.int32 and torch.equal(back, pairs)
    _, fbound = check_against_reference(X, layers, cu, H, d, scale, pairs, f'contact_features {name}')
    # the per-sequence list form gives the same rows
    per_seq = [pairs[pairs[:, 0] == s][:, 1:].long() for s in range(len(MODEL_LENGTHS))]
    X2, pairs2 = model.contact_features(tokens, (cu, ml), pairs=per_seq)
    order = torch.cat([(pairs[:, 0] == s).nonzero().reshape(-1) for s in range(len(MODEL_LENGTHS))])
    assert torch.equal(pairs2, pairs[order]) and torch.equal(X2, X[order])
    # predict_contacts with a random head (w, b) against b + X . w
    head = _random_head(L, H)
    model.set_contact_head(head)
    try:
        logit = model.predict_contacts(tokens, (cu, ml), logits=True, _keep_qk=True)
        torch.cuda.synchronize()
        for (q, k, qp), (q2, k2, qp2) in zip(layers, _captured(model, L)):
            assert torch.equal(q, q2) and torch.equal(k, k2) and qp == qp2
    finally:
        model.contact_head = None
    w = head.regression.weight.detach().to(DEV).reshape(L, H)
    cbound = CB.contact_bound(layers, cu, H, d, scale, w, BIAS)
    w64 = w.double().reshape(-1)
    lin = BIAS + X.double() @ w64
    s, i, j = (pairs[:, c].long() for c in range(3))
    worst = 0.0
    for b in range(len(MODEL_LENGTHS)):
        sel = (s == b).nonzero().reshape(-1)
        if sel.numel():
            allowed = cbound[b][i[sel], j[sel]] + fbound[sel] @ w64.abs()
            worst = max(worst, float(((logit[b][i[sel], j[sel]].double() - lin[sel]).abs() / allowed).max()))
    print(f'{name}: predict_contacts logits against b + X . w: worst err / bound {worst:.3f}')
    assert worst <= 1.0


def test_all_pairs_min_sep_and_padded_tokens():
    model = _model('esm2')
    tokens, cu, ml = _batch()
    X, pairs = model.contact_features(tokens, (cu, ml), min_sep=6)
    n = [max(m - 2, 0) for m in MODEL_LENGTHS]
    assert pairs.device == X.device and pairs.dtype == torch.int32
    assert pairs.shape[0] == sum((m - 6) * (m - 5) // 2 for m in n if m > 6) and bool((pairs[:, 2] - pairs[:, 1] >= 6).all())
    assert pairs.unique(dim=0).shape[0] == pairs.shape[0] and bool(torch.isfinite(X).all())
    X0, pairs0 = model.contact_features(tokens, (cu, ml))
    assert pairs0.shape[0] == sum(m * (m - 1) // 2 for m in n) and bool((pairs0[:, 2] > pairs0[:, 1]).all())
    keep = (pairs0[:, 2] - pairs0[:, 1] >= 6).nonzero().reshape(-1)
    assert torch.equal(pairs0[keep], pairs) and torch.equal(X0[keep], X)
    # 2-D tokens
    pad = model.alphabet.padding_idx
    grid = torch.full((len(MODEL_LENGTHS), ml + 3), pad, dtype=tokens.dtype, device=DEV)
    cul = cu.tolist()
    for s, m in enumerate(MODEL_LENGTHS):
        grid[s, :m] = tokens[cul[s]:cul[s + 1]]
    Xg, pg = model.contact_features(grid, min_sep=6)
    assert torch.equal(pg, pairs) and torch.equal(Xg, X)


def test_lora_adapters_change_the_features():
    model = _model('esm2-lora')
    kind, L, E, H = MODELS['esm2-lora']
    tokens, cu, ml = _batch()
    pairs = FB.make_pairs(MODEL_LENGTHS, seed=2, random_pairs=60).to(DEV)
    X, _ = model.contact_features(tokens, (cu, ml), pairs=pairs, lora_names=['a'], _keep_qk=True)
    torch.cuda.synchronize()
    layers = _captured(model, L)
    check_against_reference(X, layers, cu, H, model.head_pad, (E // H) ** -0.5, pairs, 'contact_features with LoRA')
    base, _ = _model('esm2').contact_features(tokens, (cu, ml), pairs=pairs)
    assert not torch.equal(X, base) and float((X - base).abs().max()) > 1e-4, 'the adapters have no effect on the features'
    with pytest.raises(KeyError):
        model.contact_features(tokens, (cu, ml), pairs=pairs, lora_names=['nope'])


def test_fit_contact_head_end_to_end():
    from esme import fit_contact_head
    model = _model('esmc')
    kind, L, E, H = MODELS['esmc']
    tokens, cu, ml = _batch()
    d, scale = model.head_pad, (E // H) ** -0.5
    X, pairs = model.contact_features(tokens, (cu, ml), min_sep=6)
    # labels drawn from a planted head's own probabilities (weights sized to the features: logits of order 1)
    g = torch.Generator().manual_seed(12)
    w_plant = (torch.randn(L * H, generator=g, dtype=torch.float64) / X.double().std(0).cpu()).to(DEV)
    z = (X.double() - X.double().mean(0)) @ w_plant * (L * H) ** -0.5 * 3 - 0.5
    y = (torch.rand(z.shape, generator=g, dtype=torch.float64).to(DEV) < torch.sigmoid(z)).float()
    assert 0.1 < float(y.mean()) < 0.9
    maps = []
    s, i, j = (pairs[:, c].long() for c in range(3))
    for b, m in enumerate(MODEL_LENGTHS):
        cm = torch.full((max(m - 2, 0),) * 2, -1.0, device=DEV)
        sel = s == b
        cm[i[sel], j[sel]] = y[sel]
        cm[j[sel], i[sel]] = y[sel]
        maps.append(cm)
    head = fit_contact_head(model, [(tokens, (cu, ml))], maps, min_sep=6, tol=1e-5, max_iter=3000)
    info = head.fit_info
    print(f"fit on {pairs.shape[0]} pairs: {info['iterations']} iterations, residual {info['residual']:.3e}, objective {info['objective']:.6f}, "
          f"{int((info['weight'] != 0).sum())} of {L * H} weights non-zero")
    assert info['objective'] < float(-(y.mean() * torch.log(y.mean()) + (1 - y.mean()) * torch.log(1 - y.mean())))     # better than the intercept alone
    assert int((info['weight'] != 0).sum()) > 0
    model.set_contact_head(head)
    try:
        logit = model.predict_contacts(tokens, (cu, ml), logits=True, _keep_qk=True)
        layers = _captured(model, L)
        prob = model.predict_contacts(tokens, (cu, ml))
        torch.cuda.synchronize()
    finally:
        model.contact_head = None
    w = head.regression.weight.detach().to(DEV).reshape(L, H)
    bias = float(head.regression.bias)
    w64 = w.double().reshape(-1)
    lin = bias + X.double() @ w64
    fbound = FB.feature_bound(layers, cu, H, d, scale, pairs)
    cbound = CB.contact_bound(layers, cu, H, d, scale, w, bias)
    worst = worst_p = 0.0
    for b in range(len(MODEL_LENGTHS)):
        sel = (s == b).nonzero().reshape(-1)
        if sel.numel():
            allowed = cbound[b][i[sel], j[sel]] + fbound[sel] @ w64.abs()
            worst = max(worst, float(((logit[b][i[sel], j[sel]].double() - lin[sel]).abs() / allowed).max()))
            # sigmoid has slope <= 1 / 4; its fp32 evaluation is allowed 2 ulp at 1 (2^-22)
            worst_p = max(worst_p, float(((prob[b][i[sel], j[sel]].double() - torch.sigmoid(lin[sel])).abs() / (0.25 * allowed + 2.0 ** -22)).max()))
    print(f'fitted head: logits worst err / bound {worst:.3f}, probabilities {worst_p:.3f}')
    assert worst <= 1.0 and worst_p <= 1.0


def test_refusals():
    model = _model('esm2')
    tokens, cu, ml = _batch()
    try:
        for mode in ('half', 'exact', 'high'):
            model.set_precision(mode)
            with pytest.raises(NotImplementedError, match='precision'):
                model.contact_features(tokens, (cu, ml))
    finally:
        model.set_precision('fast')
    with pytest.raises(NotImplementedError, match='contact_features'):
        model.graphed(tokens, (cu, ml), what='contact_features')
    for bad in ([[0, 0, 31]], [[3, 0, 0]], [[5, 0, 0]], [[0, -1, 2]]):
        with pytest.raises(ValueError, match='out of range'):
            model.contact_features(tokens, (cu, ml), pairs=torch.tensor(bad))


def test_default_forward_launches_nothing_new(monkeypatch):
    """The library calls of model.forward, and the per-kernel trace of its module loop, are the same before and after a contact_features call."""
    from esme import _hip
    model = _model('esm2')
    tokens, cu, ml = _batch()
    lib = _hip.load()

    def calls():
        seen = []

        class Recorder:
            def __getattr__(self, name):
                fn = getattr(lib, name)
                if not name.startswith('esme_hip_') or not callable(fn):
                    return fn

                def wrapped(*a):
                    seen.append(name)
                    return fn(*a)
                return wrapped
        with monkeypatch.context() as mp:
            mp.setattr(_hip, '_lib', Recorder())
            out = model(tokens, (cu, ml))
            mp.setattr(_hip, 'TRACE', [])
            model(tokens, (cu, ml))
            trace = [(op, meta) for op, meta, *_ in _hip.TRACE]
        torch.cuda.synchronize()
        return seen, trace, out

    before, trace_before, out_before = calls()
    assert before and trace_before and not any('contact' in n for n in before) and not any('contact' in op for op, _ in trace_before)
    model.contact_features(tokens, (cu, ml), min_sep=6)
    after, trace_after, out_after = calls()
    assert after == before and trace_after == trace_before and torch.equal(out_before, out_after)
