"""LoRA fine-tuning on the device: one masked-token training step of the two fixture models (tiny ESM-2: E = 128, H = 4, d = 32; tiny
ESM-C: E = 128, H = 2, d = 64; the g13 adapters) through forward_trainable + esme.loss.cross_entropy, judged against the oracle's
float64 autograd (tests/golden/g14_lora_grad.npz, made by tests/golden/make_golden_lora_grad.py).

The bar per parameter tensor, in relative Frobenius error against the float64 gradient, is 2 x the error of the reference's own bf16
gradient against its fp32 gradient, read from the fixture here: both are independent bf16 pipelines against the same truth, and their
errors are of that size each.  The measured values are printed per tensor (profiles/lora_train_parity.txt keeps a run's output).
Then what the feature promises: unselected adapters and base weights get no gradient, the LM head trains when asked, forward_trainable
computes what model(...) computes, a few optimiser steps lower the loss and reach the inference forward, save_lora / load_lora carry
the result to a fresh model, and the inference paths' derived weights stay in place."""
import pytest
import torch

import esme
from golden_util import load_golden, rel_fro
from test_lora_gpu import golden_model
from test_model_gpu import assert_parity

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KINDS = ('esm2', 'esmc')


def _batch(g, kind):
    return (g[f'{kind}_tokens_in'].to(DEV), g[f'{kind}_tokens'].to(DEV), g[f'{kind}_mask'].to(DEV), (g['cu_lens'].to(DEV), int(g['max_len'])))


def _step(model, g, kind, lora_names=None):
    tokens_in, tokens, mask, pad_args = _batch(g, kind)
    model.zero_grad(set_to_none=True)
    logits = model.forward_trainable(tokens_in, pad_args, lora_names=lora_names)
    assert logits.grad_fn is not None and logits.dtype == torch.bfloat16 and logits.shape == (tokens.numel(), model.vocab_size)
    loss = esme.cross_entropy(logits, tokens, mask, alphabet=model.alphabet)
    loss.backward()
    return loss


@pytest.mark.parametrize('head', (False, True), ids=('adapters', 'adapters+lm_head'))
@pytest.mark.parametrize('kind', KINDS)
def test_loss_and_gradients_against_float64_autograd(tmp_path, kind, head):
    model, _ = golden_model(tmp_path, kind)
    g = load_golden('g14_lora_grad.npz')
    model.mark_lmhead(head)
    model.train()
    loss = _step(model, g, kind)
    truth = g[f'{kind}_oracle/loss']
    bar = 2 * abs(g[f'{kind}_ref_bf16/loss'] - g[f'{kind}_ref_f32/loss']) / abs(g[f'{kind}_ref_f32/loss'])
    err = abs(float(loss.detach()) - truth) / abs(truth)
    print(f'\n[lora-train] {kind} loss {float(loss.detach()):.5f} (float64 {truth:.5f}): error {err:.2e}, bar {bar:.2e}')
    failures = [] if err <= bar else [('loss', err, bar)]
    seen = 0
    for name, p in model.named_parameters():
        trained = '.lora_' in name or (head and name.startswith('lm_head.'))
        if not trained:
            assert p.grad is None and not p.requires_grad, f'{name}: a frozen weight got a gradient'
            continue
        seen += 1
        assert p.grad is not None and p.grad.dtype == p.dtype and bool(torch.isfinite(p.grad.float()).all()), name
        if name.startswith('lm_head.'):
            bar = 2 * g[f'{kind}_ref_bf16_error/{name}']
        else:
            bar = 2 * rel_fro(g[f'{kind}_ref_bf16/{name}'].float(), g[f'{kind}_ref_f32/{name}'])
        err = rel_fro(p.grad.float().cpu(), g[f'{kind}_oracle/{name}'])
        print(f'[lora-train] {kind} {name:48s} error {err:.4f}  bar {bar:.4f}  ({err / bar:.2f})')
        if err > bar:
            failures.append((name, err, bar))
    assert seen == len([k for k in g if k.startswith(f'{kind}_oracle/') and ('.lora_' in k or (head and '/lm_head.' in k))])
    assert not failures, failures


@pytest.mark.parametrize('kind', KINDS)
def test_only_the_selected_adapters_get_gradients(tmp_path, kind):
    model, _ = golden_model(tmp_path, kind)
    g = load_golden('g14_lora_grad.npz')
    full = {}
    _step(model.train(), g, kind)
    for n, p in model.named_parameters():
        if '.lora_' in n:
            full[n] = p.grad.clone()
    loss_a = _step(model, g, kind, lora_names=['a'])
    for n, p in model.named_parameters():
        if '.lora_' not in n:
            assert p.grad is None
        elif n.endswith('.a'):
            assert p.grad is not None and bool(p.grad.any()), n
            assert not torch.equal(p.grad, full[n]), f'{n}: the gradient ignores the selection'
        else:
            assert p.grad is None or not bool(p.grad.any()), f"{n}: adapter 'b' was not selected"
    model.eval()                                                      # the same in eval(): no dropout, nothing mode-dependent
    assert torch.equal(_step(model, g, kind, lora_names=['a']), loss_a)


@pytest.mark.parametrize('kind', KINDS)
def test_forward_trainable_computes_the_inference_forward(tmp_path, kind):
    model, g13 = golden_model(tmp_path, kind)
    tokens, pad_args = g13[f'{kind}_tokens'].to(DEV), (g13['cu_lens'].to(DEV), int(g13['max_len']))
    ref = model(tokens, pad_args)
    att = model.layers[0].self_attn
    keys = {n: att._derived.key(n) for n in ('pack', 'fold', 'lora')}
    ptrs = [t.data_ptr() for t in att._derived.tensors()]
    model.train()
    y = model.forward_trainable(tokens, pad_args)
    y.float().square().mean().backward()
    assert_parity(y.detach(), g13[f'{kind}_logits_ab_f32'], g13[f'{kind}_logits_ab_bf16'], f'{kind} forward_trainable against the reference')
    # ... and against model(...): assert_parity's floor between two bf16 pipelines.  (Not its first term with model(...) in the reference's
    # place: the fused inference forward rounds less often than the reference's data flow, which forward_trainable follows, so its error
    # against fp32 is smaller than the reference's own -- 9.2e-3 against 1.14e-2 on the ESM-C fixture, forward_trainable 1.24e-2.)
    e_ref = rel_fro(g13[f'{kind}_logits_ab_bf16'].float(), g13[f'{kind}_logits_ab_f32'])
    e_pipe = rel_fro(y.detach().float().cpu(), ref.float().cpu())
    print(f'[parity] {kind} forward_trainable against model(...): {e_pipe:.3e} (reference bf16 against fp32: {e_ref:.3e})')
    assert e_pipe <= min(max(2e-2, 1.6 * e_ref), 2.5e-2), (kind, e_pipe, e_ref)
    assert_parity(model.forward_trainable(tokens, pad_args, lora_names=['b']).detach(), g13[f'{kind}_logits_b_f32'], g13[f'{kind}_logits_b_bf16'],
                  f"{kind} forward_trainable, lora_names=['b']")
    rep = model.forward_trainable(tokens, pad_args, logits=False)
    assert rep.shape == (tokens.numel(), model.embed_dim) and rep.grad_fn is not None
    # the 2-D path: the packed rows, padded before the head as in model(tokens2d)
    tok2d = g13[f'{kind}_tokens2d'].to(DEV)
    y2d = model.forward_trainable(tok2d).detach()
    keep = tok2d.ne(model.alphabet.padding_idx)
    assert y2d.shape == (*tok2d.shape, model.vocab_size) and torch.equal(y2d[keep], y.detach())
    model.eval()
    assert rel_fro(y2d[~keep].float(), model(tok2d)[~keep].float()) < 2e-2                   # pad rows hold head(0), as there
    # building W^T for the backward left the inference paths' derived weights in place
    assert {n: att._derived.key(n) for n in keys} == keys and [t.data_ptr() for t in att._derived.tensors()] == ptrs
    assert torch.equal(model(tokens, pad_args), ref)


def test_ten_adamw_steps_train_save_and_load(tmp_path):
    kind = 'esm2'
    model, g13 = golden_model(tmp_path, kind)
    g = load_golden('g14_lora_grad.npz')
    tokens, pad_args = g13[f'{kind}_tokens'].to(DEV), (g13['cu_lens'].to(DEV), int(g13['max_len']))
    before = model(tokens, pad_args).clone()
    model.train()
    with pytest.raises(NotImplementedError, match='inference only'):
        model(tokens, pad_args)
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=5e-3, weight_decay=0.0)
    losses = []
    for _ in range(10):
        losses.append(float(_step(model, g, kind).detach()))
        opt.step()
    print(f'\n[lora-train] ten AdamW steps: loss {losses[0]:.4f} -> {losses[-1]:.4f}')
    assert losses[-1] < losses[0], losses
    model.eval()
    after = model(tokens, pad_args)
    assert not torch.equal(after, before) and rel_fro(after, before) > 1e-2
    path = str(tmp_path / 'trained.safetensors')
    model.save_lora(path)
    fresh, _ = golden_model(tmp_path, kind)
    assert torch.equal(fresh(tokens, pad_args), before)
    from test_lora_gpu import tiny
    fresh = tiny(tmp_path, kind, *(int(g13[f'{kind}_{k}']) for k in ('L', 'E', 'H', 'seed'))).load_lora(path)
    assert torch.equal(fresh(tokens, pad_args), after)
