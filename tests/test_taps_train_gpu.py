"""Training through layer taps on the device: forward_trainable(logits=False, layers=[...]) of two fixture models (3 layers, E = 128,
2 heads of dim 64; ESM-2 and ESM-C) on six packed sequences of 1, 2, 63, 64, 65 and 129 tokens, judged against the oracle's float64
representation and autograd (tests/golden/g17_taps_grad.npz and g17_taps_grad_esmc.npz, made by tests/golden/make_golden_taps_grad.py).

Values: the first E columns are the bits of forward_trainable(logits=False); each tap block is within 2 x the error of the same data
flow in bfloat16 torch ops against float64 (relative Frobenius error: the bar construction of tests/test_full_train_gpu.py).
Gradients of sum(w * rep) over all (1 + k) E columns, w fixed and random: the LoRA tensors (rank 4) and, in a second case, the
projections and LayerNorms that mark_trainable(layers=[-1]) selects, each within 2 x the bf16 flow's error for that tensor.  The
measured values are printed per tensor (profiles/taps_train_parity.txt keeps a run's output).  Then the structure, without a
tolerance: a tap of layer 0 alone sends nothing to the later layers, layer checkpointing changes no bit, and a sequence's rows do not
depend on what it is packed with."""
import numpy as np
import pytest
import torch

from golden_util import load_golden, rel_fro
from test_lora_gpu import tiny

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KINDS = ('esm2', 'esmc')
_G = {}


def _golden():
    if not _G:
        _G.update(load_golden('g17_taps_grad.npz'))
        _G.update(load_golden('g17_taps_grad_esmc.npz'))
    return _G


def _model(tmp_path, kind):
    g = _golden()
    return tiny(tmp_path, kind, int(g['L']), int(g['E']), int(g['H']), int(g[f'{kind}_seed']))


def _lora_model(tmp_path, kind):
    g = _golden()
    model = _model(tmp_path, kind).add_lora(rank=int(g['rank']), alpha=int(g['alpha']), layers=('query', 'value', 'output'))
    model.mark_only_lora_as_trainable()
    names = {n for n, _ in model.named_parameters() if '.lora_' in n}
    assert names == {k.split('/', 1)[1] for k in g if k.startswith(f'{kind}_lora/')}
    with torch.no_grad():
        for n, p in model.named_parameters():
            if '.lora_' in n:
                p.copy_(g[f'{kind}_lora/{n}'].to(DEV))
    return model.train()


def _batch(kind):
    g = _golden()
    return g[f'{kind}_tokens'].to(DEV), (g['cu_lens'].to(DEV), int(g['max_len']))


def _weights(T, C):
    """make_golden_taps_grad.loss_weights: the same numbers from the same seed."""
    return torch.from_numpy(np.random.Generator(np.random.PCG64(int(_golden()['w_seed']))).standard_normal((T, C), dtype=np.float32)).to(DEV)


def _step(model, kind, layers, w=None, **kw):
    tokens, pad_args = _batch(kind)
    model.zero_grad(set_to_none=True)
    rep = model.forward_trainable(tokens, pad_args, logits=False, layers=layers, **kw)
    E = model.embed_dim
    assert rep.grad_fn is not None and rep.dtype == torch.bfloat16 and rep.shape == (tokens.numel(), (1 + len(layers)) * E)
    w = _weights(*rep.shape) if w is None else w
    loss = (rep.float() * w).sum()
    loss.backward()
    return loss.detach(), rep.detach()


def _grads(model):
    return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('kind', KINDS)
def test_tap_values(tmp_path, kind):
    g = _golden()
    model = _model(tmp_path, kind).mark_trainable(layers=[-1]).train()
    tokens, pad_args = _batch(kind)
    E, layers = model.embed_dim, [int(i) for i in g['layers']]
    rep = model.forward_trainable(tokens, pad_args, logits=False, layers=layers)
    assert rep.shape == (tokens.numel(), 3 * E) and rep.grad_fn is not None and rep.is_contiguous()
    assert torch.equal(rep[:, :E], model.forward_trainable(tokens, pad_args, logits=False))
    truth = g[f'{kind}_taps'].double() * 2.0 ** int(g[f'{kind}_taps_exp'])
    failures = []
    for j, layer in enumerate(layers):
        bar = 2 * float(g[f'{kind}_taps_bf16_error'][j])
        err = rel_fro(rep[:, (1 + j) * E:(2 + j) * E].detach().float().cpu(), truth[:, j * E:(j + 1) * E])
        print(f'\n[taps-train] {kind} tap of layer {layer}: error {err:.4f}  bar {bar:.4f}  ({err / bar:.2f})')
        if err > bar:
            failures.append((layer, err, bar))
    assert not failures, failures
    # the listed layers in the model's order, as forward_representation(layers=) gives them
    assert torch.equal(model.forward_trainable(tokens, pad_args, logits=False, layers=[2, 0]), rep)
    assert torch.equal(model.forward_trainable(tokens, pad_args, logits=False, layers=[]), rep[:, :E])
    # the pad path: (B, S, 3 E), the packed rows where the tokens are, zeros elsewhere
    cu = pad_args[0].tolist()
    tok2d = torch.full((len(cu) - 1, pad_args[1]), model.alphabet.padding_idx, dtype=torch.int64, device=DEV)
    for i, (a, b) in enumerate(zip(cu[:-1], cu[1:])):
        tok2d[i, :b - a] = tokens[a:b]
    rep2d = model.forward_trainable(tok2d, logits=False, layers=layers)
    keep = tok2d.ne(model.alphabet.padding_idx)
    assert rep2d.shape == (*tok2d.shape, 3 * E) and rep2d.grad_fn is not None and torch.equal(rep2d[keep], rep)
    assert not bool(rep2d[~keep][:, E:].any())
    indices = torch.nonzero(keep.flatten()).flatten()
    assert torch.equal(model.forward_trainable(tokens, pad_args, pad_output=True, pad_indices=indices, logits=False, layers=layers), rep2d)
    with pytest.raises(ValueError, match='logits=False'):
        model.forward_trainable(tokens, pad_args, layers=[0])
    with pytest.raises(AssertionError, match='Invalid layer indices'):
        model.forward_trainable(tokens, pad_args, logits=False, layers=[3])


def _judge(model, kind, case, want_of):
    g = _golden()
    failures, seen = [], 0
    for name, p in model.named_parameters():
        if f'{kind}_{case}_bf16_error/{name}' not in g:
            assert p.grad is None, f'{name}: not trained in this case, but it got a gradient'
            continue
        seen += 1
        assert p.grad is not None and p.grad.dtype == p.dtype == torch.bfloat16 and bool(torch.isfinite(p.grad.float()).all()), name
        bar = 2 * g[f'{kind}_{case}_bf16_error/{name}']
        err = rel_fro(p.grad.float().cpu(), want_of(name))
        print(f'[taps-train] {kind} {case:4s} {name:48s} error {err:.4f}  bar {bar:.4f}  ({err / bar:.2f})')
        if err > bar:
            failures.append((name, err, bar))
    assert seen == len([k for k in g if k.startswith(f'{kind}_{case}_bf16_error/')]) > 0
    assert not failures, failures


@pytest.mark.parametrize('kind', KINDS)
def test_lora_gradients_against_float64_autograd(tmp_path, kind):
    g = _golden()
    model = _lora_model(tmp_path, kind)
    print()
    _step(model, kind, [int(i) for i in g['layers']])
    _judge(model, kind, 'lora', lambda name: g[f'{kind}_lora_oracle/{name}'])


@pytest.mark.parametrize('kind', KINDS)
def test_top_layer_gradients_against_float64_autograd(tmp_path, kind):
    g = _golden()
    model = _model(tmp_path, kind).mark_trainable(layers=[-1]).train()
    print()
    _step(model, kind, [int(i) for i in g['layers']])
    _judge(model, kind, 'top', lambda name: g[f'{kind}_top_oracle/{name}'].double() * 2.0 ** int(g[f'{kind}_top_oracle_exp/{name}']))


@pytest.mark.parametrize('kind', KINDS)
def test_a_tap_of_layer_0_sends_nothing_to_later_layers(tmp_path, kind):
    model = _model(tmp_path, kind).mark_trainable().train()
    tokens, _ = _batch(kind)
    E = model.embed_dim
    w = _weights(tokens.numel(), 2 * E)
    w[:, :E] = 0                                                           # nothing flows back from the final LayerNorm's block
    _step(model, kind, [0], w=w)
    reached = 0
    for name, p in model.named_parameters():
        if name.startswith('layers.0.'):
            reached += int(p.grad is not None and bool(p.grad.any()))
        elif name.startswith('layers.') or name.startswith('emb_layer_norm_after.'):
            assert p.grad is None or not bool(p.grad.any()), f'{name}: behind the tap, but its gradient is not zero'
    assert reached > 8


@pytest.mark.parametrize('adapters', (False, True), ids=('full', 'lora'))
@pytest.mark.parametrize('kind', KINDS)
def test_layer_checkpointing_is_bit_equal_with_taps(tmp_path, kind, adapters):
    model = _lora_model(tmp_path, kind) if adapters else _model(tmp_path, kind).mark_trainable().train()
    loss, rep = _step(model, kind, [0, 2])
    plain = _grads(model)
    loss_c, rep_c = _step(model, kind, [0, 2], checkpoint_layers=True)
    ckpt = _grads(model)
    assert torch.equal(loss, loss_c) and torch.equal(rep, rep_c) and set(plain) == set(ckpt) and len(plain) >= 18
    for n in plain:
        assert torch.equal(plain[n], ckpt[n]), n


@pytest.mark.parametrize('kind', KINDS)
def test_a_sequence_alone_and_packed_gives_the_same_rows(tmp_path, kind):
    model = _lora_model(tmp_path, kind)
    tokens, (cu, max_len) = _batch(kind)
    packed = model.forward_trainable(tokens, (cu, max_len), logits=False, layers=[0, 2]).detach()
    cu = cu.tolist()
    for s in range(len(cu) - 1):
        a, b = cu[s], cu[s + 1]
        alone = model.forward_trainable(tokens[a:b], (torch.tensor([0, b - a], dtype=torch.int32, device=DEV), b - a), logits=False, layers=[0, 2])
        assert torch.equal(alone.detach(), packed[a:b]), f'sequence {s} ({b - a} tokens)'
