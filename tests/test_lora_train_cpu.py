"""LoRA fine-tuning without a GPU: esme.loss against torch's losses, the consistency of the gradient fixture (tests/golden/g14_lora_grad.npz:
the reference's fp32 gradients, taken through the corrected rotary seam, equal the oracle's float64 autograd), the refusals of
forward_trainable that need no device, the transposed-weight cache, and the inference forward still refusing train mode."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_util import GOLDEN, load_golden, rel_fro

KINDS = ('esm2', 'esmc')
PAD = (torch.tensor([0, 4], dtype=torch.int32), 4)
TOK = torch.full((4,), 5, dtype=torch.long)


# ------------------------------------------------------------------ esme.loss

@pytest.mark.parametrize('shape', [(37,), (3, 11)])
def test_losses_equal_torch(shape):
    import esme
    from esme import loss as L
    from esme.alphabet import Alphabet, Alphabet3
    assert esme.cross_entropy is L.cross_entropy and esme.nll_loss is L.nll_loss
    g = torch.Generator().manual_seed(len(shape))
    V = 33
    logits = torch.randn(*shape, V, generator=g, requires_grad=True)
    tokens = torch.randint(4, 24, shape, generator=g)
    mask = torch.rand(shape, generator=g) < 0.4
    tokens.view(-1)[mask.view(-1).nonzero()[0]] = Alphabet3.padding_idx            # one masked target is padding: ignored
    assert Alphabet.padding_idx == Alphabet3.padding_idx
    keep = mask.view(-1)
    want = F.cross_entropy(logits.view(-1, V)[keep], tokens.view(-1)[keep], ignore_index=Alphabet3.padding_idx)
    got = L.cross_entropy(logits, tokens, mask)
    assert torch.equal(got, want) and got.grad_fn is not None
    no_ignore = F.cross_entropy(logits.view(-1, V)[keep], tokens.view(-1)[keep])
    assert not torch.equal(no_ignore, want)
    logp = torch.log_softmax(logits, -1)
    assert torch.equal(L.nll_loss(logp, tokens, mask), F.nll_loss(logp.view(-1, V)[keep], tokens.view(-1)[keep], ignore_index=Alphabet3.padding_idx))
    assert torch.allclose(L.nll_loss(logp, tokens, mask), want, atol=1e-6)
    # the kwargs reach torch's loss; another alphabet's padding index is honoured
    s = L.cross_entropy(logits, tokens, mask, cross_entropy_loss_kwargs={'reduction': 'sum'})
    assert torch.allclose(s, want * int((keep & (tokens.view(-1) != Alphabet3.padding_idx)).sum()), rtol=1e-5)
    assert torch.equal(L.nll_loss(logp, tokens, mask, nll_loss_kwargs={'reduction': 'none'}),
                       F.nll_loss(logp.view(-1, V)[keep], tokens.view(-1)[keep], ignore_index=1, reduction='none'))


# ------------------------------------------------------------------ the fixture

def test_fixture_is_consistent():
    path = os.path.join(GOLDEN, 'g14_lora_grad.npz')
    assert os.path.getsize(path) < 1_000_000
    g = load_golden('g14_lora_grad.npz')
    g13 = load_golden('g13_lora.npz')
    for kind in KINDS:
        assert torch.equal(g[f'{kind}_tokens'], g13[f'{kind}_tokens'])
        mask = g[f'{kind}_mask']
        assert mask.dtype == torch.bool and int(mask.sum()) == round(0.3 * mask.numel())
        assert bool((g[f'{kind}_tokens_in'][mask] == 32).all()) and torch.equal(g[f'{kind}_tokens_in'][~mask], g[f'{kind}_tokens'][~mask])
        assert abs(g[f'{kind}_ref_f32/loss'] - g[f'{kind}_oracle/loss']) < 1e-6 * g[f'{kind}_oracle/loss'] + 1e-6
        names = sorted(k.split('/', 1)[1] for k in g if k.startswith(f'{kind}_oracle/') and not k.endswith('/loss'))
        adapters = [n for n in names if '.lora_' in n]
        head = [n for n in names if n.startswith('lm_head.')]
        assert len(adapters) + len(head) == len(names) and len(head) == 6
        assert len(adapters) == {'esm2': 2 * 3 * 2 * 2, 'esmc': 2 * 4 * 2 * 2}[kind]
        for n in adapters:
            ref32, ref16, orc = g[f'{kind}_ref_f32/{n}'], g[f'{kind}_ref_bf16/{n}'], g[f'{kind}_oracle/{n}']
            assert ref16.dtype == torch.bfloat16 and ref32.shape == ref16.shape == orc.shape
            e = rel_fro(ref32, orc)
            assert e < 1e-5, (kind, n, e)                          # the reference (corrected rotary seam) against float64 autograd
            bar = rel_fro(ref16.float(), ref32)
            assert 1e-3 < bar < 0.1, (kind, n, bar)                # a bf16 pipeline's own error: what the GPU test's bar is made of
        for n in head:
            assert 1e-3 < g[f'{kind}_ref_bf16_error/{n}'] < 0.1


# ------------------------------------------------------------------ refusals that need no device

def _model(cls=None, **kw):
    from esme import ESM2
    return (cls or ESM2)(**{'num_layers': 1, 'embed_dim': 128, 'attention_heads': 4, **kw})


def test_inference_forward_still_refuses_train_mode():
    m = _model().add_lora(rank=4, alpha=4)
    m.train()
    with pytest.raises(NotImplementedError, match='inference only'):
        m(TOK, PAD)
    from esme.lora import LoRA
    with pytest.raises(NotImplementedError, match='inference only'):
        m.layers[0].self_attn.q(torch.zeros(2, 128, dtype=torch.bfloat16))
    assert isinstance(m.layers[0].self_attn.q, LoRA)


def test_forward_trainable_refuses_by_name():
    from esme import ESM1b, ESM2, ESMC
    for m, pat in ((_model(embed_dim=480, attention_heads=20), 'padded layout'),
                   (_model(embed_dim=64, attention_heads=4), 'head dim 16'),
                   (_model(embed_dim=256, attention_heads=2), 'head dim 128'),
                   (_model().add_lora(rank=4, alpha=4, dropout_p=0.1), 'dropout'),
                   (_model(ESMC, attention_heads=2).add_lora(rank=4, alpha=4, dropout_p=0.5), 'dropout')):
        for mode in (m.train, m.eval):
            mode()
            with pytest.raises(NotImplementedError, match=pat):
                m.forward_trainable(TOK, PAD)
    m = _model().add_lora(rank=4, alpha=4)
    for precision in ('high', 'half', 'exact'):
        m.precision = precision
        with pytest.raises(NotImplementedError, match='precision'):
            m.forward_trainable(TOK, PAD)
    m.precision = 'fast'
    m.quantization = '4bit'
    with pytest.raises(NotImplementedError, match='quantised'):
        m.forward_trainable(TOK, PAD)
    m.quantization = None
    m.layers[0]._q4_up = object()
    with pytest.raises(NotImplementedError, match='quantised'):
        m.layers[0].forward_trainable(torch.zeros(4, 128, dtype=torch.bfloat16), *PAD)
    m.layers[0]._q4_up = None
    m.layers[0].self_attn._q4_qkv = object()
    with pytest.raises(NotImplementedError, match='quantised'):
        m.forward_trainable(TOK, PAD)
    m.layers[0].self_attn._q4_qkv = None
    with pytest.raises(KeyError, match='nope'):
        m.forward_trainable(TOK, PAD, lora_names=['nope'])
    with pytest.raises(NotImplementedError, match='learned-position'):
        ESM1b(num_layers=1, embed_dim=128, attention_heads=2).forward_trainable(TOK, PAD)
    with pytest.raises(RuntimeError, match='no CPU fallback'):           # every check passed: the first kernel call says where it must run
        m.forward_trainable(TOK, PAD)


# ------------------------------------------------------------------ the derived-weight cache

def test_transposed_weight_has_a_key_of_its_own():
    from esme.nn import bump_weights_epoch, weight_t
    m = _model()
    att = m.layers[0].self_attn
    pack = att._pack()
    key = att._derived.key('pack')
    wt = weight_t(att.q)
    assert wt.is_contiguous() and torch.equal(wt, att.q.weight.data.t())
    assert weight_t(att.q) is wt                                             # cached
    assert att._derived.key('pack') == key and att._pack()[0] is pack[0]     # the inference path's derived weights stay in place
    assert set(att._derived._entries) == {'pack'}
    with torch.no_grad():
        att.q.weight.mul_(2.0)                                               # an in-place edit moves the version counter
    wt2 = weight_t(att.q)
    assert wt2 is not wt and torch.equal(wt2, att.q.weight.data.t())
    bump_weights_epoch()
    assert weight_t(att.q) is not wt2
