"""LoRA adapters on the device: esme_hip_lora_down alone and the extended GEMMs against float64 within the per-element bound of
tests/lora_bounds.py (no rms floor), the models against the reference's own outputs (tests/golden/g13_lora*: made by
tests/golden/make_golden_lora.py from files the reference's save_lora wrote), and the identities the feature promises: fresh adapters
(lora_B = 0) change no bit, a sequence alone equals the same sequence in a packed batch, adapter selection and in-place edits of
lora_B take effect.  Reads tests/golden/ only."""
import os

import numpy as np
import pytest
import torch

import error_bounds as eb
import lora_bounds as lb
from golden_util import GOLDEN, load_golden
from oracle import esm_oracle as O
from esme import ESM, synthetic as syn, _hip
from test_model_gpu import assert_parity

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = {'none': None, 'a': ['a'], 'b': ['b'], 'ab': ['a', 'b']}


def rnd(rng, *shape, scale=1.0):
    return torch.from_numpy(rng.standard_normal(shape, dtype=np.float32) * scale).bfloat16()


def tiny(tmp_path, kind, L, E, H, seed):
    path = syn.write_checkpoint(str(tmp_path / f'{kind}_{L}_{E}_{H}_{seed}.safetensors'), f'{kind}_t', L, E, H, seed=seed)
    return ESM.from_pretrained(path, device=DEV)


def golden_model(tmp_path, kind):
    g = load_golden('g13_lora.npz')
    model = tiny(tmp_path, kind, *(int(g[f'{kind}_{k}']) for k in ('L', 'E', 'H', 'seed')))
    return model.load_lora(os.path.join(GOLDEN, f'g13_lora_{kind}.safetensors')), g


def fill_b(model, seed, scale=0.1):
    gen = torch.Generator(device='cpu').manual_seed(seed)
    with torch.no_grad():
        for k, p in sorted(model.named_parameters()):
            if '.lora_B.' in k:
                p.copy_((torch.randn(p.shape, generator=gen) * scale / p.shape[1] ** 0.5).to(p.dtype))


# ---------------------------------------------------------------------------------------------------------------------
# the kernel alone

SHAPES = [(320, 64, 1), (320, 128, 17), (640, 64, 129), (640, 128, 1000), (1152, 64, 333), (1152, 128, 64), (1280, 64, 50000),
          (1280, 128, 4097), (2560, 64, 127), (2560, 128, 50000), (1280, 192, 257), (1280, 256, 130)]


@pytest.mark.parametrize('ln', [False, True], ids=['plain', 'layernorm'])
@pytest.mark.parametrize('E,X,T', SHAPES)
def test_lora_down_vs_float64(E, X, T, ln):
    """u against float64 on the operands handed to the kernel, per element; rank < X: the columns past it are zero; the output is a
    strided column block between canary columns, which stay untouched."""
    rng = np.random.Generator(np.random.PCG64(E + X + T))
    R = X - 11 if T % 2 else X                                     # ragged rank on the odd shapes
    x = (rnd(rng, T, E).float() * (0.5 + rnd(rng, 1, E).float().abs()) + rnd(rng, 1, E, scale=0.5).float()).bfloat16().to(DEV)
    A = rnd(rng, R, E, scale=E ** -0.5).to(DEV)
    left, right = 8, 24
    buf = torch.full((T, left + X + right), 7.0, dtype=torch.bfloat16, device=DEV)
    u = buf[:, left:left + X]
    if ln:
        gamma, beta = (1 + rnd(rng, E, scale=0.2).float()).bfloat16().to(DEV), rnd(rng, E, scale=0.3).to(DEV)
        Ap = (A.float() * gamma.float()).bfloat16().contiguous()
        c1, bA = Ap.float().sum(1).contiguous(), (A.float() @ beta.float()).contiguous()
        sums = _hip.row_sums(x)
        _hip.lora_down(x, Ap, u, ln=(sums, E, 1e-5, c1, bA))
        ref, bound, _ = lb.down_reference(x, Ap, sums, E, 1e-5, c1, bA)
    else:
        _hip.lora_down(x, A, u)
        ref, bound, _ = lb.down_reference(x, A)
    torch.cuda.synchronize()
    assert bool((buf[:, :left] == 7.0).all()) and bool((buf[:, left + X:] == 7.0).all()), 'columns beside the extension tile were written'
    assert not bool(u[:, R:].any()), 'columns past the active ranks must be zero'
    worst = eb.assert_bounded(u[:, :R], ref, bound, f'lora_down E={E} X={X} T={T} ln={ln}')
    print(f'\n[lora_down] E={E} X={X} T={T} rank rows {R} ln={ln}: worst err / bound {worst:.3f}')


def test_lora_down_in_place_next_to_x():
    """The model's layout: u is the column block E .. E+X of the buffer whose first E columns are x; x is left as it was."""
    rng = np.random.Generator(np.random.PCG64(3))
    T, E, X = 777, 640, 64
    xe = torch.zeros(T, E + X, dtype=torch.bfloat16, device=DEV)
    xe[:, :E] = rnd(rng, T, E).to(DEV)
    before = xe[:, :E].clone()
    A = rnd(rng, 48, E, scale=E ** -0.5).to(DEV)
    _hip.lora_down(xe[:, :E], A, xe[:, E:])
    assert torch.equal(xe[:, :E], before)
    ref, bound, _ = lb.down_reference(before, A)
    eb.assert_bounded(xe[:, E:E + 48], ref, bound, 'lora_down next to x')


# ---------------------------------------------------------------------------------------------------------------------
# the extended GEMMs

@pytest.mark.parametrize('E,H,T,ranks', [(1280, 20, 1500, (16, 16)), (640, 20, 700, (16, 16, 16, 16, 16, 16)), (320, 20, 333, (8,))])
def test_extended_qkv_gemm_vs_float64(E, H, T, ranks):
    """LayerNorm-folded QKV GEMM over [x | u] with rotary and the q pre-scale in its epilogue, judged (i) as a GEMM on the operands it was
    handed (u as esme_hip_lora_down_ln wrote it), with the rotary bound on top, and (ii) before rotary end to end against the float64
    statement of the reference's data flow, within lora_bounds.qkv_reference's bound."""
    from esme.attention import _fold_layernorm, _q_scale
    rng = np.random.Generator(np.random.PCG64(E + T))
    d = E // H
    x = (rnd(rng, T, E).float() * (0.5 + rnd(rng, 1, E).float().abs()) + rnd(rng, 1, E, scale=0.3).float()).bfloat16()
    W, bias = rnd(rng, 3 * E, E, scale=E ** -0.5), rnd(rng, 3 * E, scale=0.1)
    gamma, beta = (1 + rnd(rng, E, scale=0.2).float()).bfloat16(), rnd(rng, E, scale=0.3)
    projs = ('q', 'k', 'v')[:max(1, min(3, len(ranks)))] if len(ranks) < 6 else ('q', 'k', 'v')
    names = tuple(f'n{i}' for i in range(max(1, len(ranks) // len(projs))))
    r, s = ranks[0], 1.5
    adapters = {n: {p: (rnd(rng, r, E, scale=E ** -0.5), rnd(rng, E, r, scale=0.5 * r ** -0.5)) for p in projs} for n in names}
    A, sB = lb.stack(adapters, names, projs, E, s)
    R, X = A.shape[0], lb.ext_width(A.shape[0])
    wf, c1, c2 = _fold_layernorm(W.to(DEV), bias.to(DEV), gamma.to(DEV), beta.to(DEV))
    Ap = (A.float() * gamma.float()).bfloat16().to(DEV).contiguous()
    c1A, bA = Ap.float().sum(1).contiguous(), (A.float() @ beta.float()).to(DEV).contiguous()
    we = torch.zeros(3 * E, E + X, dtype=torch.bfloat16, device=DEV)
    we[:, :E] = wf
    we[:, E:E + R] = sB.float().bfloat16().to(DEV)
    xe = torch.empty(T, E + X, dtype=torch.bfloat16, device=DEV)
    xe[:, :E] = x.to(DEV)
    sums = _hip.row_sums(xe[:, :E])
    _hip.lora_down(xe[:, :E], Ap, xe[:, E:], ln=(sums, E, 1e-5, c1A, bA))
    plain = _hip.gemm_fused(xe, we, None, ln=(sums, E, 1e-5, c1, c2, None))
    # (ii) end to end, before rotary
    ref, bound, _, _ = lb.qkv_reference(x, W, bias, gamma, beta, 1e-5, adapters, names, projs, s, sums=sums.cpu())
    worst = eb.assert_bounded(plain.cpu(), ref, bound, f'extended QKV end to end E={E}')
    delta = lb.delta64(x, gamma, beta, 1e-5, adapters, names, projs, s)
    print(f'\n[lora qkv] E={E} T={T} rank rows {R} (X={X}): worst err / bound {worst:.3f}; median |delta| / bound '
          f'{float((delta.abs() / bound).median()):.1f}')
    # (i) with rotary + q pre-scale, as a GEMM on the operands handed to it
    lengths = [T // 3, T - T // 3]
    cu = syn.cu_lens_of(lengths).to(DEV)
    pos, _ = _hip.seq_positions(cu, T)
    cos, sin = O.rotary_tables(max(lengths), d, torch.bfloat16)
    qs = _q_scale(d) if d in (32, 64) else 0.0
    got = _hip.gemm_fused(xe, we, None, ln=(sums, E, 1e-5, c1, c2, None), rot=(cos.to(DEV), sin.to(DEV), pos, d, 2 * E), q_scale=qs)
    y, pre = eb.ln_fold_reference(xe.cpu(), we.cpu(), c1.cpu(), c2.cpu(), 1e-5, sums=sums.cpu(), dim=E)
    out_ref, out_pre = y.clone(), pre.clone()
    for blk, scale in ((slice(0, E), qs or None), (slice(E, 2 * E), None)):
        rr, re = eb.rotary_bound(y[:, blk].reshape(T, H, d), pre[:, blk].reshape(T, H, d), cos, sin, pos.cpu(), q_scale=scale)
        out_ref[:, blk], out_pre[:, blk] = rr.reshape(T, E), re.reshape(T, E)
    eb.assert_bounded(got.cpu(), out_ref, out_pre + eb.out_round(out_ref, out_pre, 'bf16'), f'extended QKV + rotary E={E}')


@pytest.mark.parametrize('E,T,R', [(1280, 1500, 16), (640, 333, 96), (1152, 700, 33)])
def test_extended_out_projection_vs_float64(E, T, R):
    """Out-projection over [a | u] with the residual epilogue and row statistics: the result against float64 on the operands handed
    to it, and the statistics it emits against the row sums of what it wrote."""
    rng = np.random.Generator(np.random.PCG64(E + T + R))
    X = lb.ext_width(R)
    a = rnd(rng, T, E).to(DEV)
    A = rnd(rng, R, E, scale=E ** -0.5).to(DEV)
    W, bias, resid = rnd(rng, E, E, scale=E ** -0.5).to(DEV), rnd(rng, E, scale=0.1).to(DEV), rnd(rng, T, E).to(DEV)
    sB = rnd(rng, E, R, scale=0.3 * R ** -0.5).to(DEV)
    ae = torch.empty(T, E + X, dtype=torch.bfloat16, device=DEV)
    ae[:, :E] = a
    _hip.lora_down(ae[:, :E], A, ae[:, E:])
    we = torch.zeros(E, E + X, dtype=torch.bfloat16, device=DEV)
    we[:, :E], we[:, E:E + R] = W, sB
    stats = torch.empty(_hip.stats_blocks(T, E), T, 2, dtype=torch.float32, device=DEV)
    alpha = 0.75
    out = _hip.gemm_fused(ae, we, bias, _hip.EPI_RESIDUAL, resid, alpha, stats_out=stats)
    ref, bound, _ = eb.gemm_reference(ae.cpu(), we.cpu(), bias.cpu(), 'residual', resid.cpu(), alpha)
    worst = eb.assert_bounded(out.cpu(), ref, bound, f'extended out-projection E={E}')
    u_ref, u_bound, _ = lb.down_reference(a.cpu(), A.cpu())
    eb.assert_bounded(ae[:, E:E + R].cpu(), u_ref, u_bound, 'its down-projection')
    delta = (u_ref @ sB.double().cpu().T).abs() * alpha
    print(f'\n[lora out] E={E} T={T} R={R}: worst err / bound {worst:.3f}; median |delta| / bound {float((delta / bound).median()):.1f}')
    s = stats.sum(0).double().cpu()
    o = out.double().cpu()
    assert torch.allclose(s[:, 0], o.sum(1), rtol=1e-4, atol=1e-3) and torch.allclose(s[:, 1], (o * o).sum(1), rtol=1e-4, atol=1e-3)


# ---------------------------------------------------------------------------------------------------------------------
# models against the reference's outputs

@pytest.mark.parametrize('kind', ['esm2', 'esmc'])
def test_models_vs_reference_every_selection(kind, tmp_path):
    model, g = golden_model(tmp_path, kind)
    tokens, cu, ml = g[f'{kind}_tokens'].to(DEV), g['cu_lens'].to(DEV), int(g['max_len'])
    outs = {}
    for case, names in CASES.items():
        y = model(tokens, (cu, ml), lora_names=names)
        assert y.dtype == torch.bfloat16 and y.is_contiguous()
        assert_parity(y, g[f'{kind}_logits_{case}_f32'], g[f'{kind}_logits_{case}_bf16'], f'{kind} lora_names={names}')
        outs[case] = y
    assert torch.equal(outs['none'], outs['ab']) and torch.equal(outs['none'], model(tokens, (cu, ml), lora_names=[]))
    assert not torch.equal(outs['a'], outs['b'])
    y2d = model(g[f'{kind}_tokens2d'].to(DEV))
    assert_parity(y2d, g[f'{kind}_logits2d_none_f32'], g[f'{kind}_logits2d_none_bf16'], f'{kind} 2-D input, all adapters')
    lp = model.predict_log_prob(tokens, (cu, ml), lora_names=['a'])
    assert_parity(lp, torch.log_softmax(g[f'{kind}_logits_a_f32'], -1), torch.log_softmax(g[f'{kind}_logits_a_bf16'].float(), -1).bfloat16(),
                  f'{kind} predict_log_prob a')
    pr = model.predict_prob(tokens, pad_args=(cu, ml), lora_names=['b']).float().cpu()
    assert torch.allclose(pr.sum(-1), torch.ones(pr.shape[0]), atol=2e-2)
    rep = model.forward_representation(tokens, (cu, ml), lora_names=['a'], layers=[0])
    assert rep.shape == (tokens.numel(), 2 * model.embed_dim) and rep.is_contiguous()
    assert torch.equal(model.lm_head(rep[:, :model.embed_dim].contiguous()), outs['a'])
    with pytest.raises(KeyError):
        model(tokens, (cu, ml), lora_names=['nope'])


@pytest.mark.parametrize('kind', ['esm2', 'esmc'])
def test_layer0_taps_vs_reference(kind, tmp_path):
    model, g = golden_model(tmp_path, kind)
    tokens, cu, ml = g[f'{kind}_tokens'].to(DEV), g['cu_lens'].to(DEV), int(g['max_len'])
    att = model.layers[0].self_attn
    x0 = model.embedding(tokens, (cu, ml))
    T, E = x0.shape
    with _hip.stream_scope(DEV):
        q, k, v = att._qkv(x0, ['a', 'b'])
        for nm, t in (('q', q), ('k', k), ('v', v)):
            assert_parity(t.reshape(T, E), g[f'{kind}_tap_{nm}_f32'], g[f'{kind}_tap_{nm}_bf16'], f'{kind} layer 0 {nm} with adapters')
        ctx = model._context(cu, ml, T, x0.device)
        o_fold = att(x0, cu, ml, None, ctx, x_stats=_hip.row_sums(x0))
        o_plain = att(x0, cu, ml, ['a', 'b'], ctx)
    for what, o in (('LayerNorm-folded', o_fold), ('unfolded', o_plain)):
        assert_parity(o, g[f'{kind}_tap_attn_out_f32'], g[f'{kind}_tap_attn_out_bf16'], f'{kind} layer 0 attention branch, {what}')


# ---------------------------------------------------------------------------------------------------------------------
# identities

GEOMETRIES = [('esm2', 2, 64, 4), ('esm2', 2, 128, 4), ('esm2', 2, 128, 2), ('esm2', 2, 320, 20), ('esmc', 2, 128, 2), ('esmc', 2, 192, 3)]


@pytest.mark.parametrize('kind,L,E,H', GEOMETRIES)
@pytest.mark.parametrize('n_adapters', [1, 2], ids=['X64', 'X128'])
def test_fresh_adapters_change_no_bit(kind, L, E, H, n_adapters, tmp_path):
    """lora_B = 0 after add_lora: logits bit-identical to the same model without adapters (packed and 2-D), in every geometry, with
    extension widths 64 and 128 on the QKV GEMM."""
    lengths = [31, 7, 150, 64]
    tokens, cu = syn.random_tokens(lengths, 5).to(DEV), syn.cu_lens_of(lengths).to(DEV)
    tok2d = torch.full((len(lengths), max(lengths)), 1, dtype=torch.int64)
    for i, (a, b) in enumerate(zip(cu[:-1].tolist(), cu[1:].tolist())):
        tok2d[i, :b - a] = tokens[a:b].cpu()
    base = tiny(tmp_path, kind, L, E, H, 9)
    want, want2d = base(tokens, (cu, max(lengths))), base(tok2d.to(DEV))
    rep = base.forward_representation(tokens, (cu, max(lengths)), layers=[0, 1])
    model = tiny(tmp_path, kind, L, E, H, 9)
    names = ['a', 'b'][:n_adapters]                     # 3 projections x rank 16 x 1 or 2 adapters: 48 -> X = 64, 96 -> X = 128
    model.add_lora(rank=16, alpha=24, layers=('query', 'key', 'value', 'output'), adapter_names=names)
    assert model.layers[0].self_attn.lora_ext_widths(None)[0] == 64 * n_adapters
    assert torch.equal(model(tokens, (cu, max(lengths))), want)
    assert torch.equal(model(tokens, (cu, max(lengths)), lora_names=names[:1]), want)
    assert torch.equal(model(tok2d.to(DEV)), want2d)
    assert torch.equal(model.forward_representation(tokens, (cu, max(lengths)), layers=[0, 1]), rep)
    fill_b(model, 1)
    assert not torch.equal(model(tokens, (cu, max(lengths))), want)


def test_three_adapters_on_one_model(tmp_path):
    """Three named adapters: each selection differs, order of names does not matter beyond rounding, all == None."""
    lengths = [40, 9, 77]
    tokens, cu = syn.random_tokens(lengths, 2).to(DEV), syn.cu_lens_of(lengths).to(DEV)
    model = tiny(tmp_path, 'esm2', 2, 128, 4, 4)
    model.add_lora(rank=5, alpha=7, layers=('query', 'value', 'output'), adapter_names=['x', 'y', 'z'])
    fill_b(model, 3, scale=1.0)
    run = lambda names: model(tokens, (cu, 77), lora_names=names)
    outs = {n: run([n]) for n in 'xyz'}
    assert len({tuple(o.flatten().tolist()[:64]) for o in outs.values()}) == 3
    assert torch.equal(run(None), run(['x', 'y', 'z']))
    assert float((run(['z', 'x']).float() - run(['x', 'z']).float()).abs().max()) <= 0.25      # same sum, another column order


@pytest.mark.parametrize('kind', ['esm2', 'esmc'])
def test_alone_equals_packed_with_adapters(kind, tmp_path):
    model, g = golden_model(tmp_path, kind)
    lengths = [33, 150, 70, 1, 260]
    tokens, cu = syn.random_tokens(lengths, 8).to(DEV), syn.cu_lens_of(lengths).to(DEV)
    packed = model(tokens, (cu, max(lengths)), lora_names=['a', 'b'])
    cul = cu.tolist()
    for i, n in enumerate(lengths):
        alone = model(tokens[cul[i]:cul[i + 1]], (torch.tensor([0, n], dtype=torch.int32, device=DEV), n), lora_names=['a', 'b'])
        assert torch.equal(alone, packed[cul[i]:cul[i + 1]]), f'sequence {i} (length {n}) differs alone vs packed'


def test_selection_switch_and_in_place_edit(tmp_path):
    model, g = golden_model(tmp_path, 'esm2')
    tokens, cu, ml = g['esm2_tokens'].to(DEV), g['cu_lens'].to(DEV), int(g['max_len'])
    a1 = model(tokens, (cu, ml), lora_names=['a'])
    b1 = model(tokens, (cu, ml), lora_names=['b'])
    a2 = model(tokens, (cu, ml), lora_names=['a'])
    assert torch.equal(a1, a2) and not torch.equal(a1, b1)
    p = model.layers[1].self_attn.v.lora_B['a']
    keep = p.detach().clone()
    with torch.no_grad():
        p.mul_(1.5)
    a3 = model(tokens, (cu, ml), lora_names=['a'])
    assert not torch.equal(a3, a1), 'an in-place edit of lora_B must reach the next forward'
    assert torch.equal(model(tokens, (cu, ml), lora_names=['b']), b1), "adapter 'b' is untouched"
    with torch.no_grad():
        p.copy_(keep)
    assert torch.equal(model(tokens, (cu, ml), lora_names=['a']), a1), 'restoring lora_B restores the bits'


def test_refusals_on_the_device(tmp_path):
    model, g = golden_model(tmp_path, 'esm2')
    tokens, cu, ml = g['esm2_tokens'].to(DEV), g['cu_lens'].to(DEV), int(g['max_len'])
    with pytest.raises(NotImplementedError, match='graph'):
        model.graphed(tokens, (cu, ml))
    for mode in ('half', 'exact', 'high'):
        with pytest.raises(NotImplementedError):
            model.set_precision(mode)
    model.train()
    with pytest.raises(NotImplementedError, match='inference only'):
        model(tokens, (cu, ml))
    model.eval()
    q8 = ESM.from_pretrained(syn.write_checkpoint(str(tmp_path / 'q.safetensors'), 'esm2_q', 2, 128, 4, seed=1), quantization='4bit', device=DEV)
    with pytest.raises(NotImplementedError, match='quanti'):
        q8.add_lora()


def test_full_size_esm2_650m_50k_rank16():
    """ESM2-650M geometry, 33 layers, 50 000 residues, one rank-16 adapter on q / v / out: three whole sequences against the oracle's
    forward on weights with the delta s B A applied in fp32 by this test (the oracle itself is untouched), under the rule of
    tests/test_fullsize_gpu.py (parity + alone-vs-packed bit equality)."""
    from test_fullsize_gpu import load, check_sequences
    model, w, H = load('esm2_650m')
    model.add_lora(rank=16, alpha=16, layers=('query', 'value', 'output'), adapter_names=['ft'])
    fill_b(model, 17, scale=0.5)
    w = dict(w)
    for i, layer in enumerate(model.layers):
        for p in ('q', 'v', 'out'):
            m = getattr(layer.self_attn, p)
            key = f'layers.{i}.self_attn.{p}.weight'
            w[key] = w[key].float() + m.scaling * (m.lora_B['ft'].detach().float().cpu() @ m.lora_A['ft'].detach().float().cpu())
    tokens, cu, max_len, lengths = syn.uniform_batch(50000, 500, seed=0)
    out = check_sequences(model, w, H, tokens, cu, max_len, [0, 57, 99], 'ESM2-650M 33 layers, 50 000 residues, LoRA rank 16 on q / v / out')
    assert out.shape == (50000, model.vocab_size)
