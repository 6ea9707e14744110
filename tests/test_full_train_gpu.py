"""Full fine-tuning on the device: one masked-token training step of the two fixture models without adapters (tiny ESM-2: E = 128,
H = 4, d = 32; tiny ESM-C: E = 128, H = 2, d = 64, SwiGLU) through mark_trainable + forward_trainable + esme.loss.cross_entropy, judged
against the oracle's float64 autograd (tests/golden/g15_full_grad.npz and g15_full_grad_esmc.npz, made by
tests/golden/make_golden_full_grad.py).

The bar per parameter tensor, in relative Frobenius error against the float64 gradient, is 2 x the error of the same data flow in
bfloat16 torch ops against that truth, read from the fixture here: two independent bf16 pipelines against one truth err by that size
each.  The measured values are printed per tensor (profiles/full_train_parity.txt keeps a run's output).  Then what the feature
promises: layer selection, the frozen path's bits, the routing of every trainable projection through esme_hip_gemm_wgrad (and of nothing
else), bit-equal gradients under layer checkpointing, optimiser steps that lower the loss and reach the inference forward, and the
refusal of a trainable token embedding."""
import pytest
import torch

import esme
from golden_util import load_golden, rel_fro
from test_lora_gpu import golden_model, tiny

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KINDS = ('esm2', 'esmc')
PROJECTIONS = {'esm2': 6, 'esmc': 7}          # per layer: q, k, v, out and FFN up / down, or SwiGLU's two and the down-projection
_G = {}


def _golden():
    if not _G:
        _G.update(load_golden('g15_full_grad.npz'))
        _G.update(load_golden('g15_full_grad_esmc.npz'))
        _G['g13'] = load_golden('g13_lora.npz')
    return _G


def _model(tmp_path, kind):
    g13 = _golden()['g13']
    return tiny(tmp_path, kind, *(int(g13[f'{kind}_{k}']) for k in ('L', 'E', 'H', 'seed')))


def _step(model, kind, **kw):
    g = _golden()
    tokens_in, tokens, mask = (g[f'{kind}_{k}'].to(DEV) for k in ('tokens_in', 'tokens', 'mask'))
    model.zero_grad(set_to_none=True)
    logits = model.forward_trainable(tokens_in, (g['cu_lens'].to(DEV), int(g['max_len'])), **kw)
    assert logits.dtype == torch.bfloat16 and logits.shape == (tokens.numel(), model.vocab_size)
    loss = esme.cross_entropy(logits, tokens, mask, alphabet=model.alphabet)
    loss.backward()
    return loss.detach()


def _is_backbone(name):
    return (name.startswith('layers.') or name.startswith('emb_layer_norm_after.')) and '.lora_' not in name


def _grads(model):
    return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


class _Recorder:
    """The loaded library with every esme_hip_* call counted by name."""

    def __init__(self, lib):
        self.lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith('esme_hip_') or not callable(fn):
            return fn

        def wrapped(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return wrapped


def _record(monkeypatch):
    from esme import _hip, _hip_attn_bwd, _hip_gemm_wgrad
    lib = _hip.load()
    _hip_gemm_wgrad.bind(lib)
    _hip_attn_bwd.bind(lib)
    rec = _Recorder(lib)
    monkeypatch.setattr(_hip, '_lib', rec)
    return rec


@pytest.mark.parametrize('kind', KINDS)
def test_loss_and_gradients_against_float64_autograd(tmp_path, kind):
    g = _golden()
    model = _model(tmp_path, kind).mark_trainable().train()
    loss = float(_step(model, kind))
    truth = g[f'{kind}_oracle/loss']
    bar = 2 * g[f'{kind}_bf16_error/loss']
    err = abs(loss - truth) / abs(truth)
    print(f'\n[full-train] {kind} loss {loss:.5f} (float64 {truth:.5f}): error {err:.2e}, bar {bar:.2e}')
    failures = [] if err <= bar else [('loss', err, bar)]
    seen = 0
    for name, p in model.named_parameters():
        if not _is_backbone(name):
            assert p.grad is None and not p.requires_grad, f'{name}: a frozen weight got a gradient'
            continue
        seen += 1
        assert p.grad is not None and p.grad.dtype == p.dtype == torch.bfloat16 and bool(torch.isfinite(p.grad.float()).all()), name
        want = g[f'{kind}_oracle/{name}'].double() * 2.0 ** int(g[f'{kind}_oracle_exp/{name}'])
        bar = 2 * g[f'{kind}_bf16_error/{name}']
        err = rel_fro(p.grad.float().cpu(), want)
        print(f'[full-train] {kind} {name:44s} error {err:.4f}  bar {bar:.4f}  ({err / bar:.2f})')
        if err > bar:
            failures.append((name, err, bar))
    assert seen == len([k for k in g if k.startswith(f'{kind}_oracle_exp/')])
    assert not failures, failures


@pytest.mark.parametrize('kind', KINDS)
def test_layer_selection_and_the_frozen_path(tmp_path, kind):
    g = _golden()
    model = _model(tmp_path, kind).train()
    tokens_in, pad_args = g[f'{kind}_tokens_in'].to(DEV), (g['cu_lens'].to(DEV), int(g['max_len']))
    frozen = model.forward_trainable(tokens_in, pad_args).clone()          # FrozenLinear everywhere: the path as it was before mark_trainable existed
    assert frozen.grad_fn is None
    _step(model.mark_trainable(layers=[1]), kind)
    for name, p in model.named_parameters():
        if name.startswith('layers.1.'):
            assert p.requires_grad and p.grad is not None and bool(p.grad.any()), name
        else:
            assert not p.requires_grad and p.grad is None, f'{name}: not selected, but it got a gradient'
    one = _grads(model)
    y = model.forward_trainable(tokens_in, pad_args)
    assert y.grad_fn is not None and torch.equal(y.detach(), frozen)       # TrainableLinear's forward is the same GEMM
    _step(model.mark_trainable(), kind)
    full = _grads(model)
    assert all(torch.equal(full[n], one[n]) for n in one)                 # a layer's gradient does not depend on what else is trained
    model.mark_trainable(False, False)
    assert not any(p.requires_grad for p in model.parameters())
    again = model.forward_trainable(tokens_in, pad_args)
    assert again.grad_fn is None and torch.equal(again, frozen)


@pytest.mark.parametrize('kind', KINDS)
def test_every_trainable_projection_goes_through_the_kernel(tmp_path, kind, monkeypatch):
    L, per = 2, PROJECTIONS[kind]
    model = _model(tmp_path, kind).train()
    rec = _record(monkeypatch)
    _step(model.mark_trainable(), kind)
    assert rec.calls.get('esme_hip_gemm_wgrad', 0) == L * per and rec.calls.get('esme_hip_attn_varlen_bwd', 0) == L, rec.calls
    rec.calls.clear()
    _step(model.mark_trainable(layers=[1]), kind)
    assert rec.calls.get('esme_hip_gemm_wgrad', 0) == per, rec.calls
    rec.calls.clear()
    _step(model.mark_trainable(projections=False), kind)                   # LayerNorms only: torch's gradients
    assert rec.calls.get('esme_hip_gemm_wgrad', 0) == 0, rec.calls
    rec.calls.clear()
    _step(model.mark_trainable(False, False).mark_lmhead(True), kind)      # the LM head keeps F.linear
    assert rec.calls.get('esme_hip_gemm_wgrad', 0) == 0, rec.calls
    assert all((p.grad is not None) == n.startswith('lm_head.') for n, p in model.named_parameters())
    monkeypatch.undo()
    # adapters: none when only they train; through the wrapper the base `layer` follows the same rule
    lora, _ = golden_model(tmp_path, kind)
    rec = _record(monkeypatch)
    _step(lora.train(), kind)
    assert rec.calls.get('esme_hip_gemm_wgrad', 0) == 0 and rec.calls.get('esme_hip_attn_varlen_bwd', 0) == L, rec.calls
    rec.calls.clear()
    _step(lora.mark_trainable(norms=False), kind)
    assert rec.calls.get('esme_hip_gemm_wgrad', 0) == L * per, rec.calls
    got = {n for n, p in lora.named_parameters() if p.grad is not None}
    assert any('.lora_A.' in n for n in got) and any(n.endswith('self_attn.q.layer.weight') for n in got)


@pytest.mark.parametrize('kind', KINDS)
def test_layer_checkpointing_is_bit_equal(tmp_path, kind):
    model = _model(tmp_path, kind).mark_trainable().train()
    loss = _step(model, kind)
    plain = _grads(model)
    loss_c = _step(model, kind, checkpoint_layers=True)
    ckpt = _grads(model)
    assert torch.equal(loss, loss_c) and set(plain) == set(ckpt) and len(plain) > 20
    for n in plain:
        assert torch.equal(plain[n], ckpt[n]), n


def test_ten_adamw_steps_reach_the_inference_forward(tmp_path):
    kind = 'esm2'
    g = _golden()
    model = _model(tmp_path, kind)
    keys = list(model.state_dict())
    tokens, pad_args = g[f'{kind}_tokens'].to(DEV), (g['cu_lens'].to(DEV), int(g['max_len']))
    before = model(tokens, pad_args).clone()
    model.mark_trainable().train()
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.0)
    losses = []
    for _ in range(10):
        losses.append(float(_step(model, kind)))
        opt.step()
    print(f'\n[full-train] ten AdamW steps at lr 1e-3: loss {losses[0]:.4f} -> {losses[-1]:.4f}')
    assert losses[-1] < losses[0], losses
    model.eval()
    after = model(tokens, pad_args)                                        # the derived-weight caches are keyed on the version counters
    assert not torch.equal(after, before) and rel_fro(after, before) > 1e-2
    trained = model.forward_trainable(tokens, pad_args).detach()
    e = rel_fro(after.float(), trained.float())
    print(f'[full-train] model(...) against forward_trainable after the steps: {e:.3e}')
    assert e <= 2.5e-2                                                     # the floor between the fused and the unfused bf16 pipelines (test_lora_train_gpu.py)
    assert list(model.state_dict()) == keys


def test_a_trainable_token_embedding_is_refused(tmp_path):
    g = _golden()
    model = _model(tmp_path, 'esm2').mark_trainable()
    model.embed_tokens.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match='mark_trainable'):
        model.forward_trainable(g['esm2_tokens_in'].to(DEV), (g['cu_lens'].to(DEV), int(g['max_len'])))
