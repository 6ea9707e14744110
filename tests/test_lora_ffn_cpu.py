"""LoRA adapters on the FFN projections ('ffn_up' / 'ffn_down' of ESM2.add_lora), the parts that need no device: which modules are
wrapped in both families, the names that stay refused, the extension widths and their limit, the layout of the extended SwiGLU
up-weight (each adapter's s B in exactly its projection's interleaved rows), the life of the derived entry, save_lora / load_lora, and the
host validation of esme_hip_lora_down at the FFN's K.  The GPU half is tests/test_lora_ffn_gpu.py."""
import ctypes

import pytest
import torch
from safetensors import safe_open
from safetensors.torch import load_file

from esme import ESM, synthetic as syn, _hip
from esme.attention import SwiGLU
from esme.lora import LoRA

KINDS = ('esm2', 'esmc')
ALL_SIX = ('query', 'key', 'value', 'output', 'ffn_up', 'ffn_down')
L, E, H = 2, 128, 2                 # F = 512 (GELU: 4 E; SwiGLU: 8/3 E rounded up to a multiple of 256)


def base_model(kind, tmp_path, seed=3):
    path = syn.write_checkpoint(str(tmp_path / f'{kind}_{seed}.safetensors'), f'{kind}_t', L, E, H, seed=seed)
    return ESM.from_pretrained(path, device='cpu')


def fill_b(model, seed, scale=0.5):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in sorted(model.named_parameters()):
            if '.lora_B.' in k:
                p.copy_((torch.randn(p.shape, generator=gen) * scale / p.shape[1] ** 0.5).to(p.dtype))


def metadata(path):
    with safe_open(path, framework='pt', device='cpu') as f:
        return dict(f.metadata())


def assert_same_file(a, b):
    """The same metadata and byte-equal tensors under the same keys in the same order.  (Not the files' own bytes: safetensors writes
    the metadata entries of its header in an order that changes from one save to the next.)"""
    assert metadata(a) == metadata(b)
    ta, tb = load_file(a), load_file(b)
    assert list(ta) == list(tb)
    for k in ta:
        assert ta[k].dtype == tb[k].dtype and ta[k].shape == tb[k].shape and torch.equal(ta[k].view(torch.int16), tb[k].view(torch.int16)), k


@pytest.mark.parametrize('kind', KINDS)
def test_ffn_names_wrap_the_ffn_projections(kind, tmp_path):
    model = base_model(kind, tmp_path)
    before = set(model.state_dict())
    assert model.add_lora(rank=4, alpha=8, layers=('ffn_up', 'ffn_down')) is model and model.has_lora
    assert model.lora_kwargs['layers'] == ['ffn_up', 'ffn_down']
    after = set(model.state_dict())
    for i, layer in enumerate(model.layers):
        att = layer.self_attn
        assert not any(isinstance(getattr(att, p), LoRA) for p in ('q', 'k', 'v', 'out')), 'the attention projections were not named'
        if kind == 'esm2':
            wrapped = {'final.1': layer.final[1], 'final.3': layer.final[3]}
        else:
            sw = layer.final[1]
            assert isinstance(sw, SwiGLU), "SwiGLU itself stays: 'ffn_up' wraps its two projections"
            wrapped = {'final.1.activation': sw.activation, 'final.1.fc': sw.fc, 'final.2': layer.final[2]}
        F = 512
        for name, m in wrapped.items():
            assert isinstance(m, LoRA) and m.rank == 4 and m.scaling == 2.0, name
            down = name in ('final.3', 'final.2')
            assert tuple(m.lora_A['default'].shape) == ((4, F) if down else (4, E)) and tuple(m.lora_B['default'].shape) == ((E, 4) if down else (F, 4))
            assert m.lora_A['default'].any() and not m.lora_B['default'].any()
            base = f'layers.{i}.{name}'
            assert f'{base}.weight' in before and f'{base}.weight' not in after and f'{base}.layer.weight' in after
            assert {f'{base}.lora_A.default', f'{base}.lora_B.default'} <= after
    assert len(model.lora_state_dict()) == L * 2 * len(wrapped)
    for k, p in model.named_parameters():
        assert p.requires_grad == ('.lora_A.' in k or '.lora_B.' in k), k
    model.mark_trainable()                                            # reaches the base projection under an FFN wrapper
    ups, down = model.layers[0]._ffn_projections()
    assert all(m.layer.weight.requires_grad for _, m in (*ups, down))
    model.mark_trainable(False, False)
    assert not any(m.layer.weight.requires_grad for _, m in (*ups, down))


def test_any_subset_of_the_six_names_and_the_names_that_stay_refused(tmp_path):
    model = base_model('esm2', tmp_path)
    for bad in (('query', 'ffn'), ('ffn',), ('ffn_up', 'up'), ('final',)):
        with pytest.raises(AssertionError):
            model.add_lora(layers=bad)
    assert not model.has_lora
    model.add_lora(rank=8, layers=('ffn_down', 'value'))
    assert model.lora_kwargs['layers'] == ['value', 'ffn_down']
    layer = model.layers[1]
    assert isinstance(layer.self_attn.v, LoRA) and isinstance(layer.final[3], LoRA) and not isinstance(layer.final[1], LoRA)
    assert layer.self_attn.lora_ext_widths(None) == (64, 0) and layer.ffn_lora_ext_widths(None) == (0, 64)
    default = base_model('esm2', tmp_path).add_lora()
    assert default.lora_kwargs['layers'] == ['query', 'value', 'output'] and default.layers[0].ffn_lora_ext_widths(None) == (0, 0)
    assert not default.layers[0]._has_lora and default.layers[0]._derived.key('lora') is None


@pytest.mark.parametrize('kind', KINDS)
def test_ext_widths_and_the_extension_limit(kind, tmp_path):
    per_up = 2 if kind == 'esmc' else 1                               # SwiGLU: two adapters of that rank in the up GEMM
    one = base_model(kind, tmp_path).add_lora(rank=16, layers=ALL_SIX)
    assert one.layers[0].ffn_lora_ext_widths(None) == (64, 64)
    three = base_model(kind, tmp_path).add_lora(rank=24, layers=ALL_SIX, adapter_names=['x', 'y', 'z'])
    layer = three.layers[0]
    assert layer.ffn_lora_ext_widths(None) == (64 * -(-3 * 24 * per_up // 64), 128)
    assert layer.ffn_lora_ext_widths(['y']) == (64, 64)
    assert layer.self_attn.lora_ext_widths(None) == (256, 128), "the attention block's two-tuple is what it was"
    with pytest.raises(KeyError):
        layer.ffn_lora_ext_widths(['nope'])
    wide = base_model(kind, tmp_path).add_lora(rank=64, layers=('ffn_up', 'ffn_down'), adapter_names=['a', 'b', 'c', 'd', 'e'])
    with pytest.raises(NotImplementedError, match='extension'):
        wide.layers[0].ffn_lora_ext_widths(None)                      # 320 stacked rows in the down GEMM (and 320 / 640 in the up GEMM)
    assert wide.layers[0].ffn_lora_ext_widths(['a', 'b']) == (128 * per_up, 128)


def test_extended_swiglu_weight_keeps_each_adapter_in_its_interleaved_rows(tmp_path):
    """[W' | s B | 0] of the SwiGLU up-projection: rows 64 j .. 64 j + 31 are the gate's rows 32 j .., rows 64 j + 32 .. 64 j + 63 fc's; the
    gate adapter's columns come first and are zero in the fc rows, fc's follow and are zero in the gate rows."""
    model = base_model('esmc', tmp_path).add_lora(rank=5, alpha=15, layers=('ffn_up',), adapter_names=['a', 'b'])
    fill_b(model, 1)
    layer = model.layers[0]
    sw = layer.final[1]
    F = sw.out_features
    for fold in (True, False):
        X, A, c1A, bA, we = layer._ffn_lora_weights(None, fold)['up']
        assert X == 64 and A.shape == (20, E) and we.shape == (2 * F, E + X) and we.dtype == torch.bfloat16
        base = layer._pack_fold()[0] if fold else sw._pack()
        assert torch.equal(we[:, :E], base), 'the base columns are the weight the adapter-free GEMM reads'
        rows = we[:, E:].view(F // 32, 2, 32, X)
        gate_rows, fc_rows = rows[:, 0].reshape(F, X), rows[:, 1].reshape(F, X)
        s = 3.0
        want_g = torch.cat([(sw.activation.lora_B[n].data.float() * s).bfloat16() for n in ('a', 'b')], 1)
        want_f = torch.cat([(sw.fc.lora_B[n].data.float() * s).bfloat16() for n in ('a', 'b')], 1)
        assert want_g.any() and want_f.any()
        assert torch.equal(gate_rows[:, :10], want_g) and torch.equal(fc_rows[:, 10:20], want_f)
        assert not gate_rows[:, 10:].any(), "the fc adapter's columns (and the pad columns) are zero in the gate rows"
        assert not fc_rows[:, :10].any() and not fc_rows[:, 20:].any(), "the gate adapter's columns (and the pad columns) are zero in the fc rows"
        want_A = torch.cat([m.lora_A[n].data for m in (sw.activation, sw.fc) for n in ('a', 'b')], 0)
        if fold:
            ln = layer.final[0]
            assert torch.equal(A, (want_A.float() * ln.weight.data.float()).bfloat16())
            assert torch.equal(c1A, A.float().sum(1)) and torch.allclose(bA, want_A.float() @ ln.bias.data.float())
        else:
            assert torch.equal(A, want_A) and c1A is None and bA is None
    # one adapter selected: its columns alone
    X, A, _, _, we = layer._ffn_lora_weights(['b'], False)['up']
    rows = we[:, E:].view(F // 32, 2, 32, X)
    assert A.shape == (10, E) and torch.equal(rows[:, 0].reshape(F, X)[:, :5], (sw.activation.lora_B['b'].data.float() * 3.0).bfloat16())
    assert torch.equal(rows[:, 1].reshape(F, X)[:, 5:10], (sw.fc.lora_B['b'].data.float() * 3.0).bfloat16()) and not we[:, E + 10:].any()


@pytest.mark.parametrize('kind', KINDS)
def test_gelu_and_down_weights_and_the_life_of_the_derived_entry(kind, tmp_path):
    model = base_model(kind, tmp_path).add_lora(rank=4, alpha=4, layers=ALL_SIX, adapter_names=['a', 'b'])
    fill_b(model, 2)
    layer = model.layers[0]
    ups, (_, down) = layer._ffn_projections()
    F = 512
    lw = layer._ffn_lora_weights(None, True)
    Xd, Ad, wd = lw['down']
    assert Xd == 64 and Ad.shape == (8, F) and wd.shape == (E, F + 64)
    assert torch.equal(wd[:, :F], down.layer.weight.data) and not wd[:, F + 8:].any()
    assert torch.equal(wd[:, F:F + 8], torch.cat([down.lora_B[n].data.float().bfloat16() for n in ('a', 'b')], 1))
    if kind == 'esm2':
        X, A, _, _, we = lw['up']
        assert we.shape == (F, E + 64) and torch.equal(we[:, :E], layer._pack_fold()[0])
        assert torch.equal(we[:, E:E + 8], torch.cat([ups[0][1].lora_B[n].data for n in ('a', 'b')], 1)) and not we[:, E + 8:].any()
    # cached: the same object until a parameter it was built from changes in place
    assert layer._ffn_lora_weights(None, True) is lw and layer._ffn_lora_weights(['a', 'b'], True) is lw
    key = layer._derived.key('lora')
    with torch.no_grad():
        layer.self_attn.q.lora_B['a'].mul_(2.0)                       # (an attention adapter: not this entry's business)
    assert layer._ffn_lora_weights(None, True) is lw and layer._derived.key('lora') == key
    with torch.no_grad():
        down.lora_B['b'].mul_(2.0)
    lw2 = layer._ffn_lora_weights(None, True)
    assert lw2 is not lw and layer._derived.key('lora') != key
    assert torch.equal(lw2['down'][2][:, F + 4:F + 8], down.lora_B['b'].data) and torch.equal(lw2['up'][4], lw['up'][4])
    assert layer._ffn_lora_weights(None, True) is lw2
    with torch.no_grad():
        ups[-1][1].lora_B['a'].add_(0.25)
    lw3 = layer._ffn_lora_weights(None, True)
    assert lw3 is not lw2 and not torch.equal(lw3['up'][4], lw2['up'][4])
    only_a = layer._ffn_lora_weights(['a'], True)                      # another selection: another entry
    assert only_a is not lw3 and only_a['down'][1].shape == (4, F)


@pytest.mark.parametrize('kind', KINDS)
def test_save_then_load_into_a_fresh_model(kind, tmp_path):
    model = base_model(kind, tmp_path).add_lora(rank=6, alpha=9, layers=ALL_SIX, adapter_names=['a', 'b'], dropout_p=0.0)
    fill_b(model, 4)
    path = str(tmp_path / 'six.safetensors')
    model.save_lora(path)
    md = metadata(path)
    assert set(md) == {'rank', 'alpha', 'dropout_p', 'layers', 'names', 'format'}
    assert md['layers'] == ','.join(ALL_SIX) and md['names'] == 'a,b' and md['rank'] == '6' and md['alpha'] == '9'
    fresh = base_model(kind, tmp_path).load_lora(path)
    a, b = model.state_dict(), fresh.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    assert fresh.lora_kwargs == model.lora_kwargs and fresh.lora_names() == ['a', 'b']
    again = str(tmp_path / 'six_again.safetensors')
    fresh.save_lora(again)
    assert_same_file(path, again)


@pytest.mark.parametrize('kind', KINDS)
def test_a_file_without_ffn_names_round_trips_byte_equal(kind, tmp_path):
    model = base_model(kind, tmp_path).add_lora(rank=8, alpha=16, layers=('query', 'value', 'output'), adapter_names=['a'])
    fill_b(model, 5)
    path = str(tmp_path / 'attn.safetensors')
    model.save_lora(path)
    assert metadata(path)['layers'] == 'query,value,output'
    assert not any('.final.' in k for k in load_file(path))
    fresh = base_model(kind, tmp_path).load_lora(path)
    assert not fresh.layers[0]._has_lora and not any(isinstance(m, LoRA) for _, m in fresh.layers[0]._ffn_projections()[0])
    again = str(tmp_path / 'attn_again.safetensors')
    fresh.save_lora(again)
    assert_same_file(path, again)


def test_refusals_reach_the_ffn_adapters(tmp_path):
    model = base_model('esm2', tmp_path).add_lora(rank=4, layers=('ffn_up', 'ffn_down'))
    for mode in ('half', 'exact', 'high'):
        with pytest.raises(NotImplementedError, match='LoRA'):
            model.set_precision(mode)
    tokens, cu = syn.random_tokens([5, 9], 1), syn.cu_lens_of([5, 9])
    with pytest.raises(NotImplementedError, match='graph'):
        model.graphed(tokens, (cu, 9))
    assert not model._c_forward_ok()
    model.train()
    with pytest.raises(NotImplementedError, match='inference only'):
        model(tokens, (cu, 9))
    layer = model.layers[0]
    x = torch.zeros(14, E, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match='inference only'):
        layer._ffn(x, 1.0, {'resid': x, 'out': x})
    model.eval()
    with pytest.raises(NotImplementedError, match="precision 'fast' only"):
        layer._ffn(x, 1.0, {'resid32': x.float(), 'out': x})
    drop = base_model('esm2', tmp_path).add_lora(rank=4, layers=('ffn_down',), dropout_p=0.1)
    with pytest.raises(NotImplementedError, match='dropout_p'):
        drop.layers[0].check_trainable()
    with pytest.raises(NotImplementedError, match='rank'):
        base_model('esm2', tmp_path).add_lora(rank=65, layers=('ffn_up',))


def test_host_validation_of_lora_down_at_the_ffn_width():
    """K = 10 240 (the widest FFN served) with ldx = K + X passes the host checks (T = 0: nothing is launched; the pointers are fake)."""
    lib = _hip.load()
    P = ctypes.c_void_p
    K = 10240
    for X, rank in ((64, 16), (128, 100), (256, 256)):
        assert lib.esme_hip_lora_down(P(4096), K + X, P(1 << 20), rank, 0, K, X, P(4096 + 2 * K), K + X, None) == 0
    assert lib.esme_hip_lora_down(P(4096), 512 + 64, P(1 << 20), 20, 0, 512, 64, P(4096 + 2 * 512), 512 + 64, None) == 0
    assert lib.esme_hip_lora_down(P(4096), K, P(1 << 20), 16, 0, K, 64, P(8192), 64, None) == 0
    assert lib.esme_hip_lora_down(P(4096), K - 8, P(1 << 20), 16, 0, K, 64, P(8192), 64, None) == -1          # ldx < K
    assert lib.esme_hip_lora_down(P(4096), K + 32, P(1 << 20), 16, 0, K + 32, 64, P(8192), 64, None) == -2    # K % 64 != 0
