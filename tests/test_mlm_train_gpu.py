"""Masked-LM training on the device: the two fixture models without adapters (tiny ESM-2: E = 128, H = 4; tiny ESM-C: E = 128, H = 2,
SwiGLU, a 64-row table) with every projection, LayerNorm AND the token embedding trained, through mark_trainable(embedding=True) +
forward_trainable + esme.loss.cross_entropy.

The embedding gradient is judged against the oracle's float64 autograd (tests/golden/g17_embed_grad.npz, made by
tests/golden/make_golden_embed_grad.py); the bar, in relative Frobenius error, is 2 x the error of the same data flow in bfloat16 torch
ops against that truth, read from the fixture: two independent bf16 pipelines against one truth err by that size each.  The measured
ratio is printed (profiles/mlm_train_parity.txt keeps a run's output).  Then what the opt-in promises: ESM-2's `<mask>` row gets an
exactly zero gradient and ESM-C's does not; every other parameter's gradient is bit-equal with and without the opt-in; loss and
gradients are bit-equal under layer checkpointing; 2-D tokens give the packed gradients; esme_hip_embed_bwd runs exactly once per
backward with the opt-in and never without; ten esme.optim.AdamW steps on MaskedFastaTokenDataset batches lower the loss, change the
table and reach the fused inference forward; and the standing refusals still raise."""
import os

import pytest
import torch

import esme
from golden_util import load_golden, rel_fro
from test_lora_gpu import tiny

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KINDS = ('esm2', 'esmc')
NAME = 'embed_tokens.weight'
FASTA = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'data', 'test.fa')
_G = {}


def _golden():
    if not _G:
        _G.update({k: v for k, v in load_golden('g15_full_grad.npz').items() if '/' not in k})      # the masked training batch
        _G.update(load_golden('g17_embed_grad.npz'))
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
    loss = esme.cross_entropy(logits, tokens, mask, alphabet=model.alphabet)
    loss.backward()
    return loss.detach()


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
    from esme import _hip, _hip_attn_bwd, _hip_embed_bwd, _hip_gemm_wgrad
    lib = _hip.load()
    for mod in (_hip_gemm_wgrad, _hip_attn_bwd, _hip_embed_bwd):
        mod.bind(lib)
    rec = _Recorder(lib)
    monkeypatch.setattr(_hip, '_lib', rec)
    return rec


@pytest.mark.parametrize('kind', KINDS)
def test_embedding_gradient_against_float64_autograd(tmp_path, kind):
    g = _golden()
    model = _model(tmp_path, kind).mark_trainable(embedding=True).train()
    loss = float(_step(model, kind))
    grad = model.embed_tokens.weight.grad
    assert grad is not None and grad.dtype == torch.bfloat16 and grad.shape == model.embed_tokens.weight.shape and bool(torch.isfinite(grad.float()).all())
    want, bar = g[f'{kind}_oracle/{NAME}'], 2 * g[f'{kind}_bf16_error/{NAME}']
    err = rel_fro(grad.float().cpu(), want)
    print(f'\n[mlm-train] {kind} loss {loss:.5f} (float64 {g[f"{kind}_oracle/loss"]:.5f})')
    print(f'[mlm-train] {kind} {NAME:44s} error {err:.4f}  bar {bar:.4f}  ({err / bar:.2f})')
    assert err <= bar
    rows = g[f'{kind}_rows']
    mask_idx = model.alphabet.mask_idx
    assert int(rows[mask_idx]) > 0
    if kind == 'esm2':                                                    # the forward zeroes <mask> rows: the table row never reaches the output
        assert not bool(grad[mask_idx].any())
    else:                                                                 # ESM-C looks <mask> up like any id: its row trains
        assert bool(grad[mask_idx].any())
    assert not bool(grad[(rows == 0).to(DEV)].any()) and bool(grad[((rows > 0) & (torch.arange(rows.numel()) != mask_idx)).to(DEV)].any(dim=1).all())


@pytest.mark.parametrize('kind', KINDS)
def test_the_other_gradients_do_not_change_and_checkpointing_is_bit_equal(tmp_path, kind):
    model = _model(tmp_path, kind).mark_trainable().train()
    loss0 = _step(model, kind)
    without = _grads(model)
    assert NAME not in without and len(without) > 20
    loss1 = _step(model.mark_trainable(embedding=True), kind)
    with_emb = _grads(model)
    assert torch.equal(loss0, loss1) and set(with_emb) == set(without) | {NAME}
    for n in without:
        assert torch.equal(with_emb[n], without[n]), n
    loss2 = _step(model, kind, checkpoint_layers=True)
    ckpt = _grads(model)
    assert torch.equal(loss2, loss1) and set(ckpt) == set(with_emb)
    for n in with_emb:
        assert torch.equal(ckpt[n], with_emb[n]), n
    _step(model.mark_trainable(False, False, embedding=True), kind)       # the table alone
    alone = _grads(model)
    assert set(alone) == {NAME} and torch.equal(alone[NAME], with_emb[NAME])
    _step(model.mark_trainable(), kind)                                   # the default withdraws the opt-in
    assert not model.embed_tokens.weight.requires_grad and model.embed_tokens.weight.grad is None


@pytest.mark.parametrize('kind', KINDS)
def test_padded_tokens_give_the_packed_gradients(tmp_path, kind):
    """2-D tokens: the same rows in a (B, S) layout with `<pad>`.  The packed rows of the logits are the same bits; the gradients may
    differ from the packed call's only where a torch GEMM of the LM head sums over another row count (the pad rows hold head(0) and
    take no gradient): far below one bf16 ulp (2^-8) in relative Frobenius error.  Pad rows contribute nothing to the table."""
    g = _golden()
    model = _model(tmp_path, kind).mark_trainable(embedding=True).train()
    _step(model, kind)
    packed = _grads(model)
    cu, S = g['cu_lens'].tolist(), int(g['max_len'])
    B, pad = len(cu) - 1, model.alphabet.padding_idx
    tok2, in2, mask2 = torch.full((B, S), pad), torch.full((B, S), pad), torch.zeros(B, S, dtype=torch.bool)
    for b, (a, e) in enumerate(zip(cu[:-1], cu[1:])):
        tok2[b, :e - a], in2[b, :e - a], mask2[b, :e - a] = g[f'{kind}_tokens'][a:e], g[f'{kind}_tokens_in'][a:e], g[f'{kind}_mask'][a:e]
    assert bool((in2 == pad).any())
    model.zero_grad(set_to_none=True)
    logits = model.forward_trainable(in2.to(DEV))
    assert logits.shape == (B, S, model.vocab_size)
    loss = esme.cross_entropy(logits, tok2.to(DEV), mask2.to(DEV), alphabet=model.alphabet)
    loss.backward()
    padded = _grads(model)
    assert set(padded) == set(packed)
    worst = max(rel_fro(padded[n].float(), packed[n].float()) for n in packed)
    equal = sum(torch.equal(padded[n], packed[n]) for n in packed)
    print(f'\n[mlm-train] {kind} 2-D tokens against packed: {equal} of {len(packed)} gradients bit-equal, worst relative difference {worst:.2e}; '
          f'table {rel_fro(padded[NAME].float(), packed[NAME].float()):.2e}')
    assert worst <= 2.0 ** -8
    assert not bool(padded[NAME][pad].any())                              # (no <pad> id in the packed batch either)


@pytest.mark.parametrize('kind', KINDS)
def test_the_kernel_runs_once_per_backward_and_only_with_the_opt_in(tmp_path, kind, monkeypatch):
    model = _model(tmp_path, kind).train()
    rec = _record(monkeypatch)
    _step(model.mark_trainable(), kind)
    assert rec.calls.get('esme_hip_embed_bwd', 0) == 0 and rec.calls.get('esme_hip_embed', 0) == 1, rec.calls
    rec.calls.clear()
    _step(model.mark_trainable(embedding=True), kind)
    assert rec.calls.get('esme_hip_embed_bwd', 0) == 1 and rec.calls.get('esme_hip_embed', 0) == 1, rec.calls
    assert rec.calls.get('esme_hip_embed_bwd_workspace_bytes', 0) == 1
    rec.calls.clear()
    _step(model, kind, checkpoint_layers=True)                            # the lookup lies outside the checkpointed layers
    assert rec.calls.get('esme_hip_embed_bwd', 0) == 1 and rec.calls.get('esme_hip_embed', 0) == 1, rec.calls
    rec.calls.clear()
    _step(model.mark_trainable(False, False, embedding=True), kind)
    assert rec.calls.get('esme_hip_embed_bwd', 0) == 1 and rec.calls.get('esme_hip_gemm_wgrad', 0) == 0, rec.calls
    rec.calls.clear()
    _step(model.mark_trainable(), kind)
    assert rec.calls.get('esme_hip_embed_bwd', 0) == 0, rec.calls


def test_ten_adamw_steps_on_masked_fasta_batches(tmp_path):
    from esme.alphabet import Alphabet
    from esme.data import MaskedFastaTokenDataset
    kind = 'esm2'
    model = _model(tmp_path, kind)
    torch.manual_seed(11)
    data = MaskedFastaTokenDataset(FASTA, token_per_batch=1000, shuffle=True, random_state=0, alphabet=Alphabet)
    batches = [data[i] for i in range(len(data))]
    assert len(batches) >= 3

    def loss_of(item, train=True):
        tokens, (cu, ml), masked, mask = item
        logits = model.forward_trainable(masked.to(DEV), (cu.to(DEV), ml))
        return esme.cross_entropy(logits, tokens.to(DEV), mask.to(DEV), alphabet=model.alphabet)

    tokens, (cu, ml), _, _ = batches[0]
    fused_before = model(tokens.to(DEV), (cu.to(DEV), ml)).clone()
    model.mark_trainable(embedding=True).mark_lmhead().train()
    w = model.embed_tokens.weight
    table_before = w.detach().clone()
    with torch.no_grad():
        held_before = float(sum(loss_of(b) for b in batches)) / len(batches)
    opt = esme.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=2e-3, weight_decay=0.0)
    losses = []
    for step in range(10):
        model.zero_grad(set_to_none=True)
        loss = loss_of(batches[step % len(batches)])
        loss.backward()
        assert w.grad is not None and bool(w.grad.any())
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        held_after = float(sum(loss_of(b) for b in batches)) / len(batches)
    print(f'\n[mlm-train] ten AdamW steps at lr 2e-3: step losses {losses[0]:.4f} -> {losses[-1]:.4f}; all batches {held_before:.4f} -> {held_after:.4f}')
    assert held_after < held_before and opt.state[w]['step'] == 10
    assert not torch.equal(w.detach(), table_before) and rel_fro(w.detach().float(), table_before.float()) > 1e-3
    assert not bool((w.detach()[model.alphabet.mask_idx] != table_before[model.alphabet.mask_idx]).any())      # a zero gradient, no weight decay: <mask> stays
    model.eval()
    fused = model(tokens.to(DEV), (cu.to(DEV), ml))                       # the fused forward reads the parameter itself
    assert rel_fro(fused.float(), fused_before.float()) > 1e-2
    trained = model.forward_trainable(tokens.to(DEV), (cu.to(DEV), ml)).detach()
    e = rel_fro(fused.float(), trained.float())
    print(f'[mlm-train] model(...) against forward_trainable after the steps: {e:.3e}')
    assert e <= 2.5e-2                                                    # the floor between the fused and the unfused bf16 pipelines (test_full_train_gpu.py)
    with torch.no_grad():                                                 # the table alone reaches the fused forward: another table, other logits
        w.mul_(0.5)
    assert rel_fro(model(tokens.to(DEV), (cu.to(DEV), ml)).float(), fused.float()) > 1e-3


def test_standing_refusals(tmp_path):
    from esme import ESM1b, ESM2
    g = _golden()
    args = (g['esm2_tokens_in'].to(DEV), (g['cu_lens'].to(DEV), int(g['max_len'])))
    model = _model(tmp_path, 'esm2').mark_trainable()
    model.embed_tokens.weight.requires_grad_(True)                        # without the opt-in: today's refusal
    with pytest.raises(NotImplementedError, match='embed_tokens.weight requires grad.*mark_trainable'):
        model.forward_trainable(*args)
    model.mark_trainable(embedding=True)
    assert model.forward_trainable(*args).grad_fn is not None
    for mode in ('high', 'half', 'exact'):                                # with the opt-in: by name
        model.precision = mode
        with pytest.raises(NotImplementedError, match=f"precision '{mode}'"):
            model.forward_trainable(*args)
    model.precision = 'fast'
    model.quantization = '4bit'
    with pytest.raises(NotImplementedError, match='quantised'):
        model.forward_trainable(*args)
    with pytest.raises(NotImplementedError, match='quantised'):
        model.mark_trainable(embedding=True)
    model.quantization = None
    padded = tiny(tmp_path, 'esm2', 1, 96, 4, 3).mark_trainable(False, False, embedding=True)
    assert padded.padded
    with pytest.raises(NotImplementedError, match='padded layout'):
        padded.forward_trainable(*args)
    esm1 = ESM1b(num_layers=1, embed_dim=128, attention_heads=2).mark_trainable(embedding=True)
    with pytest.raises(NotImplementedError, match='learned-position'):
        esm1.forward_trainable(*args)
    with pytest.raises(TypeError):
        ESM2.mark_trainable(model, embedding=True, tokens=True)
