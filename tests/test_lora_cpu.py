"""LoRA adapters, the parts that need no device: the public surface against the reference's own adapter files (tests/golden/g13_lora_*:
written by the reference's save_lora, tests/golden/make_golden_lora.py), the float64 bound of the extension-tile path against a CPU
emulation of it and against emulated defects (tests/lora_bounds.py), host validation of the new entry points, and every refusal
that can be reached without a device.  The GPU half is tests/test_lora_gpu.py."""
import ctypes
import os

import numpy as np
import pytest
import torch
from safetensors import safe_open
from safetensors.torch import load_file

import error_bounds as eb
import lora_bounds as lb
from golden_util import GOLDEN, load_golden

from esme import ESM, synthetic as syn, _hip
from esme.lora import LoRA, lora_state_dict, mark_only_lora_as_trainable

KINDS = ('esm2', 'esmc')


def fixture_path(kind):
    return os.path.join(GOLDEN, f'g13_lora_{kind}.safetensors')


def base_model(kind, tmp_path, device='cpu'):
    g = load_golden('g13_lora.npz')
    L, E, H, seed = (int(g[f'{kind}_{k}']) for k in ('L', 'E', 'H', 'seed'))
    path = syn.write_checkpoint(str(tmp_path / f'{kind}.safetensors'), f'{kind}_t', L, E, H, seed=seed)
    return ESM.from_pretrained(path, device=device), g


def metadata(path):
    with safe_open(path, framework='pt', device='cpu') as f:
        return dict(f.metadata())


@pytest.mark.parametrize('kind', KINDS)
def test_add_lora_matches_the_reference_file(kind, tmp_path):
    """Keys, shapes, dtypes and requires_grad after add_lora equal the file the reference's save_lora wrote; base weights move under .layer."""
    model, g = base_model(kind, tmp_path)
    md = metadata(fixture_path(kind))
    ref = load_file(fixture_path(kind))
    names = md['names'].split(',')
    before = set(model.state_dict())
    out = model.add_lora(rank=int(md['rank']), alpha=int(md['alpha']), layers=md['layers'].split(','), adapter_names=names)
    assert out is model and model.has_lora
    mine = model.lora_state_dict()
    assert set(mine) == set(ref)
    for k, t in ref.items():
        assert mine[k].shape == t.shape and mine[k].dtype == t.dtype == torch.bfloat16, k
        if '.lora_B.' in k:
            assert not mine[k].any(), 'lora_B starts at zero'
        else:
            assert mine[k].any(), 'lora_A is initialised'
    short = {'query': 'q', 'key': 'k', 'value': 'v', 'output': 'out'}
    wrapped = {short[l] for l in md['layers'].split(',')}
    after = set(model.state_dict())
    for p in ('q', 'k', 'v', 'out'):
        mod = getattr(model.layers[0].self_attn, p)
        assert isinstance(mod, LoRA) == (p in wrapped)
        key = f'layers.0.self_attn.{p}.layer.weight' if p in wrapped else f'layers.0.self_attn.{p}.weight'
        assert key in after and (key in before) == (p not in wrapped)
        if p in wrapped:
            assert mod.rank == int(md['rank']) and mod.alpha == int(md['alpha']) and mod.scaling == int(md['alpha']) / int(md['rank'])
            assert mod.names == set(names) and list(mod.lora_A.keys()) == names
    for k, p in model.named_parameters():
        assert p.requires_grad == ('.lora_A.' in k or '.lora_B.' in k), k
    model.mark_only_lora_as_trainable(['a'])
    for k, p in model.named_parameters():
        assert p.requires_grad == (('.lora_A.' in k or '.lora_B.' in k) and k.endswith('.a')), k
    mark_only_lora_as_trainable(model)
    assert set(lora_state_dict(model, ['b'])) == {k for k in ref if k.endswith('.b')}
    model.mark_lmhead()
    assert all(p.requires_grad for p in model.lm_head.parameters())
    model.mark_lmhead(False)
    assert not any(p.requires_grad for p in model.lm_head.parameters())


@pytest.mark.parametrize('kind', KINDS)
def test_load_then_save_roundtrip(kind, tmp_path):
    """from_pretrained of the base checkpoint + load_lora of the reference's file; save_lora writes the same metadata and byte-equal tensors."""
    model, _ = base_model(kind, tmp_path)
    assert model.load_lora(fixture_path(kind)) is model
    out = str(tmp_path / 'again.safetensors')
    model.save_lora(out)
    md0, md1 = metadata(fixture_path(kind)), metadata(out)
    assert set(md0) == set(md1) == {'rank', 'alpha', 'dropout_p', 'layers', 'names', 'format'}
    for k in md0:
        if k == 'layers':               # (the reference joins a set: its order is arbitrary)
            assert set(md0[k].split(',')) == set(md1[k].split(','))
        else:
            assert md0[k] == md1[k], k
    a, b = load_file(fixture_path(kind)), load_file(out)
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k].view(torch.int16), b[k].view(torch.int16)), k
    only_a = str(tmp_path / 'only_a.safetensors')
    model.save_lora(only_a, ['a'])
    assert set(load_file(only_a)) == {k for k in a if k.endswith('.a')} and metadata(only_a)['names'] == 'a'


def test_three_adapters_and_name_selection(tmp_path):
    model, _ = base_model('esm2', tmp_path)
    model.add_lora(rank=4, alpha=6, layers=('query', 'key'), adapter_names=['x', 'y', 'z'])
    assert model.lora_names() == ['x', 'y', 'z']
    assert model._lora_select(None) == model._lora_select([]) == ('x', 'y', 'z')
    assert model._lora_select(['z', 'x']) == ('z', 'x')
    with pytest.raises(KeyError):
        model._lora_select(['nope'])
    att = model.layers[0].self_attn
    assert att.lora_ext_widths(None) == (64, 0) and att.lora_ext_widths(['y']) == (64, 0)
    with pytest.raises(KeyError):
        att.q.select(['nope'])


def test_refusals_without_a_device(tmp_path):
    """Whatever cannot apply the adapters raises NotImplementedError and names the limit; nothing runs without them."""
    model, _ = base_model('esm2', tmp_path)
    model.set_precision('half', robust=False)
    with pytest.raises(NotImplementedError, match="precision 'half'"):
        model.add_lora()
    model.set_precision('fast')
    with pytest.raises(NotImplementedError, match='rank'):
        model.add_lora(rank=65)
    with pytest.raises(AssertionError):
        model.add_lora(layers=('query', 'ffn'))
    model.add_lora(rank=8, adapter_names=['a'])
    with pytest.raises(NotImplementedError, match='already attached'):
        model.add_lora()
    for mode in ('half', 'exact', 'high'):
        with pytest.raises(NotImplementedError, match='LoRA'):
            model.set_precision(mode)
    assert model.precision == 'fast'
    tokens, cu = syn.random_tokens([5, 9], 1), syn.cu_lens_of([5, 9])
    with pytest.raises(NotImplementedError, match='graph'):
        model.graphed(tokens, (cu, 9))
    assert not model._c_forward_ok()
    from esme import cforward
    for fn, args in ((cforward.forward_layers, (None,) * 6), (cforward.forward_layers_half, (None,) * 8), (cforward.forward_layers_exact, (None,) * 8)):
        with pytest.raises(NotImplementedError, match='LoRA'):
            fn(model, *args)
    model.train()
    with pytest.raises(NotImplementedError, match='inference only'):
        model(tokens, (cu, 9))
    model.eval()
    model.precision = 'exact'               # (set behind set_precision's back: the forward itself refuses)
    with pytest.raises(NotImplementedError, match="precision 'exact'"):
        model(tokens, (cu, 9))
    model.precision = 'fast'
    with pytest.raises(KeyError):
        model(tokens, (cu, 9), lora_names=['nope'])
    # more active adapter rows in one GEMM than the widest extension tile the kernel is built for
    wide, _ = base_model('esm2', tmp_path)
    wide.add_lora(rank=64, layers=('query', 'key', 'value'), adapter_names=['a', 'b'])
    with pytest.raises(NotImplementedError, match='extension'):
        wide.layers[0].self_attn.lora_ext_widths(None)
    assert wide.layers[0].self_attn.lora_ext_widths(['a']) == (192, 0)
    padded = ESM.from_pretrained(syn.write_checkpoint(str(tmp_path / 'p.safetensors'), 'esm2_p', 1, 96, 4, seed=3))
    assert padded.padded
    with pytest.raises(NotImplementedError, match='padded'):
        padded.add_lora()


def test_host_validation_of_the_entry_points():
    """esme_hip_lora_down / _ln check their arguments on the host (no launch happens: every pointer here is fake or null)."""
    lib = _hip.load()
    P = ctypes.c_void_p
    ok = dict(x=P(4096), ldx=128, A=P(8192), rank=16, T=10, E=128, X=64, u=P(16384), ldu=64)

    def down(**kw):
        a = {**ok, **kw}
        return lib.esme_hip_lora_down(a['x'], a['ldx'], a['A'], a['rank'], a['T'], a['E'], a['X'], a['u'], a['ldu'], None)

    def down_ln(part=P(1 << 20), nblk=1, dim=128, eps=1e-5, c1=P(1 << 21), bA=P(1 << 22), **kw):
        a = {**ok, **kw}
        return lib.esme_hip_lora_down_ln(a['x'], a['ldx'], a['A'], a['rank'], a['T'], a['E'], a['X'], a['u'], a['ldu'], part, nblk, dim, eps, c1, bA, None)

    ARG, UNS = -1, -2
    assert down(T=0) == 0 and down_ln(T=0) == 0                         # nothing to do, valid arguments
    for kw in (dict(x=None), dict(A=None), dict(u=None)):
        assert down(**kw) == ARG and b'null' in lib.esme_hip_last_error()
    assert down(X=96) == UNS and b'multiple of 64' in lib.esme_hip_last_error()
    assert down(X=320, ldu=320) == UNS and b'256' in lib.esme_hip_last_error()
    assert down(E=96, ldx=96) == UNS
    assert down(rank=65) == ARG and down(rank=0) == ARG and down(T=-1) == ARG
    assert down(ldx=120) == ARG and down(ldx=132) == ARG and down(ldu=60) == ARG and down(ldu=68) == ARG
    assert down(x=P(4098)) == ARG and down(u=P(16392)) == ARG and b'aligned' in lib.esme_hip_last_error()
    for kw in (dict(part=None), dict(c1=None), dict(bA=None), dict(nblk=0), dict(dim=0), dict(part=P((1 << 20) + 4)), dict(x=None)):
        assert down_ln(**kw) == ARG, kw


# ---------------------------------------------------------------------------------------------------------------------
# the bound: accepts a CPU emulation of the kernel path, rejects emulated defects

def _problem(seed, E=128, T=96, rank=8, alpha=12, bias=True, names=('a', 'b')):
    rng = np.random.Generator(np.random.PCG64(seed))

    def n(*shape, scale=1.0):
        return torch.from_numpy(rng.standard_normal(shape, dtype=np.float32) * scale).bfloat16()

    x = (n(T, E) * n(1, E).float().abs().add(0.5).bfloat16()).bfloat16() + n(1, E, scale=0.3)
    p = dict(x=x.bfloat16(), W=n(3 * E, E, scale=E ** -0.5), bias=n(3 * E, scale=0.1) if bias else None,
             gamma=(1.0 + n(E, scale=0.2).float()).bfloat16(), beta=n(E, scale=0.3) if bias else None, eps=1e-5, s=alpha / rank)
    p['adapters'] = {nm: {pr: (n(rank, E, scale=E ** -0.5), n(E, rank, scale=0.5 * rank ** -0.5)) for pr in ('q', 'k', 'v')} for nm in names}
    return p


def _run(p, names, projs, **kw):
    return lb.emulate_qkv(p['x'], p['W'], p['bias'], p['gamma'], p['beta'], p['eps'], p['adapters'], names, projs, p['s'], **kw)


def _ref(p, names, projs):
    return lb.qkv_reference(p['x'], p['W'], p['bias'], p['gamma'], p['beta'], p['eps'], p['adapters'], names, projs, p['s'])


@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('names,projs', [(('a',), ('q', 'k', 'v')), (('a', 'b'), ('q', 'v')), (('b',), ('k',)), ((), ())])
def test_bound_accepts_the_emulated_path(names, projs, bias):
    p = _problem(5, bias=bias)
    ref, bound, pre, _ = _ref(p, names, projs)
    worst = eb.assert_bounded(_run(p, names, projs).double(), ref, bound, f'emulated path {names} {projs}')
    print(f'\n[lora bound] emulation {names} on {projs}, bias={bias}: worst err / bound {worst:.3f}; '
          f'median bound / |ref| {float((bound / ref.abs().clamp_min(1e-3)).median()):.2e}')
    assert worst > 0.02, 'a bound fifty times the error of a faithful emulation would reject nothing'


def _rejected(got, ref, bound):
    return float(((got.double() - ref).abs() / bound).max()) > 1.0


@pytest.mark.parametrize('defect', ['no_scaling', 'inv_scaling', 'swap_qv', 'drop_key', 'no_beta'])
def test_bound_rejects_arithmetic_defects(defect):
    p = _problem(7)
    names, projs = ('a', 'b'), ('q', 'k', 'v')
    ref, bound, _, _ = _ref(p, names, projs)
    assert not _rejected(_run(p, names, projs), ref, bound)
    assert _rejected(_run(p, names, projs, defect=defect), ref, bound), defect


def test_bound_rejects_stale_cache_and_wrong_name():
    p = _problem(8)
    projs = ('q', 'k', 'v')
    ref_a, bound_a, _, _ = _ref(p, ('a',), projs)
    assert _rejected(_run(p, ('b',), projs), ref_a, bound_a), "adapter 'b' computed where 'a' was selected"
    assert _rejected(_run(p, ('a', 'b'), projs), ref_a, bound_a), 'all adapters where one was selected'
    assert _rejected(_run(p, (), ()), ref_a, bound_a), 'adapters dropped'
    old = {n: {pr: (A, B.clone()) for pr, (A, B) in d.items()} for n, d in p['adapters'].items()}
    A, B = p['adapters']['a']['v']
    p['adapters']['a']['v'] = (A, (B.float() * 1.25 + 0.01).bfloat16())            # lora_B edited in place ...
    ref_new, bound_new, _, _ = _ref(p, ('a',), projs)
    assert not _rejected(_run(p, ('a',), projs), ref_new, bound_new)
    assert _rejected(_run(p, ('a',), projs, stale=old), ref_new, bound_new), '... and a forward that still uses the cached old one'


def test_bound_rejects_delta_after_rotary_and_after_q_layernorm():
    """The delta enters BEFORE rotary (ESM-2) and before ESM-C's q LayerNorm: adding it unrotated / unnormalised afterwards is out of bound."""
    p = _problem(9)
    T, E = p['x'].shape
    H, d = 4, E // 4
    names, projs = ('a',), ('q', 'k', 'v')
    ref, bound, pre, _ = _ref(p, names, projs)
    good, base = _run(p, names, projs), _run(p, (), ())
    delta = lb.delta64(p['x'], p['gamma'], p['beta'], p['eps'], p['adapters'], names, projs, p['s'])
    cos, sin = lb.rotary_tables(T, d)
    pos = torch.arange(T)
    q = slice(0, E)
    r_ref, r_pre = eb.rotary_bound(ref[:, q].reshape(T, H, d), pre[:, q].reshape(T, H, d), cos, sin, pos)
    r_bound = r_pre + eb.out_round(r_ref, r_pre, 'bf16')

    def rot(y):
        return eb.rotary_apply64(y.double().reshape(T, H, d), cos, sin, pos).float().bfloat16()
    assert not _rejected(rot(good[:, q]), r_ref, r_bound)
    late = (rot(base[:, q]).double() + delta[:, q].reshape(T, H, d)).float().bfloat16()
    assert _rejected(late, r_ref, r_bound), 'delta added after rotary, unrotated'
    # ESM-C: q LayerNorm over the full width after the projection
    wq, bq = (1.0 + 0.1 * torch.randn(E, generator=torch.Generator().manual_seed(3))).bfloat16(), None
    n_ref, n_bound = lb.qln_reference(ref[:, q], bound[:, q], wq, bq, 1e-5)

    def qln(y):
        y = y.double()
        mu = y.mean(1, keepdim=True)
        return ((y - mu) / torch.sqrt(((y - mu) ** 2).mean(1, keepdim=True) + 1e-5) * wq.double()).float().bfloat16()
    assert not _rejected(qln(good[:, q]), n_ref, n_bound)
    assert _rejected((qln(base[:, q]).double() + delta[:, q]).float().bfloat16(), n_ref, n_bound), "delta added after ESM-C's q LayerNorm"


@pytest.mark.parametrize('ln', [False, True])
def test_down_projection_bound_accepts_an_fp32_emulation(ln):
    p = _problem(11, E=320, T=70, rank=16)
    A = torch.cat([p['adapters']['a'][pr][0] for pr in ('q', 'v')], 0)
    x = p['x']
    if not ln:
        ref, bound, _ = lb.down_reference(x, A)
        got = (x.double() @ A.double().T).float().bfloat16()
    else:
        Ap = (A.float() * p['gamma'].float()).bfloat16()
        c1, bA = Ap.float().sum(1), A.float() @ p['beta'].float()
        ref, bound, _ = lb.down_reference(x, Ap, None, None, p['eps'], c1, bA)
        x32 = x.float()
        mean = x32.mean(1, keepdim=True)
        sd = torch.sqrt(torch.clamp((x32 * x32).mean(1, keepdim=True) - mean * mean, min=0) + p['eps'])
        got = (sd * bA + ((x.double() @ Ap.double().T).float() - mean * c1)).bfloat16()
        # the value is LN(x) A^T / rstd: check the algebra against the textbook form
        h = (x.double() - x.double().mean(1, keepdim=True)) / x.double().var(1, unbiased=False, keepdim=True).add(p['eps']).sqrt() * p['gamma'].double() + p['beta'].double()
        ideal = (h @ A.double().T) * x.double().var(1, unbiased=False, keepdim=True).add(p['eps']).sqrt()
        assert float(((ref - ideal).abs() / (ideal.abs() + 1.0)).max()) < 2e-2           # (A' = bf16(gamma A) is the only difference)
    eb.assert_bounded(got.double(), ref, bound, f'lora_down emulation ln={ln}')
    assert _rejected((got.float() * 1.02).bfloat16(), ref, bound)
