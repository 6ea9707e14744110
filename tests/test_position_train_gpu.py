"""Training the learned-position models on the device: tiny ESM-1b and ESM-1v (E = 128, H = 2: head dim 64; the synthetic 4 098-row
position table) through mark_trainable(positions=...) + forward_trainable + esme.loss.cross_entropy.

The gradients of the position table (esme_hip_embed_positions_bwd), the token table, ESM-1b's emb_layer_norm_before and one projection
are judged against the oracle's float64 autograd (tests/golden/g18_position_grad.npz, made by tests/golden/make_golden_position_grad.py);
the bar, in relative Frobenius error, is 2 x the error of the same data flow in bfloat16 torch ops against that truth, read from the
fixture: two independent bf16 pipelines against one truth err by that size each.  The measured ratios are printed
(profiles/position_train_parity.txt keeps a run's output).  Then what the opt-in promises: the trainable embedding of ESM-1v is the
inference embedding bit for bit; 2-D tokens give the packed table gradient bit for bit; loss and gradients are bit-equal under layer
checkpointing and from run to run; positions='frozen' trains LoRA adapters and leaves the table without a gradient; the table alone
trains; ten esme.optim.AdamW steps lower the loss; an extended table takes a longer sequence, trains its new rows and is what the
inference forward and its graphs read afterwards; a max_len above the table is refused before any launch; and nothing on the path
synchronises the device."""
import pytest
import torch

import esme
from golden_util import load_golden, rel_fro
from test_lora_gpu import tiny

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KINDS = ('esm1b', 'esm1v')
POS, TOK, PROJ = 'embed_positions.weight', 'embed_tokens.weight', 'layers.0.self_attn.q.weight'
NORM = ('emb_layer_norm_before.weight', 'emb_layer_norm_before.bias')
_G = {}


def _golden():
    if not _G:
        _G.update({k: v for k, v in load_golden('g15_full_grad.npz').items() if '/' not in k})      # the masked training batch (ESM-2's alphabet)
        _G.update(load_golden('g18_position_grad.npz'))
    return _G


def _model(tmp_path, kind):
    g = _golden()
    return tiny(tmp_path, kind, *(int(g[k]) for k in ('L', 'E', 'H', 'seed')))


def _batch():
    g = _golden()
    return tuple(g[f'esm2_{k}'].to(DEV) for k in ('tokens_in', 'tokens', 'mask')) + (g['cu_lens'].to(DEV), int(g['max_len']))


def _step(model, **kw):
    tokens_in, tokens, mask, cu, ml = _batch()
    model.zero_grad(set_to_none=True)
    logits = model.forward_trainable(tokens_in, (cu, ml), **kw)
    loss = esme.cross_entropy(logits, tokens, mask, alphabet=model.alphabet)
    loss.backward()
    return loss.detach()


def _grads(model):
    return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('kind', KINDS)
def test_gradients_against_float64_autograd(tmp_path, kind):
    g = _golden()
    model = _model(tmp_path, kind).mark_trainable(embedding=True, positions=True).train()
    loss = float(_step(model))
    grads = _grads(model)
    print(f'\n[position-train] {kind} loss {loss:.5f} (float64 {g[f"{kind}_oracle/loss"]:.5f})')
    rows = int(g['max_len']) + 2
    table = grads[POS]
    assert table.dtype == torch.bfloat16 and table.shape == model.embed_positions.weight.shape == (4098, int(g['E']))
    fan = g[f'{kind}_fan_in']
    assert fan.numel() == rows and not bool(table[rows:].any()) and not bool(table[:2].any())          # the rows nothing reaches: exact zeros
    assert bool(table[2:rows].any(dim=1).all()) and int(fan[2]) == g['cu_lens'].numel() - 1 and int(fan[-1]) >= 1
    for name in (POS, TOK, PROJ) + (NORM if kind == 'esm1b' else ()):
        got = grads[name][:rows] if name == POS else grads[name]
        want, bar = g[f'{kind}_oracle/{name}'], 2 * g[f'{kind}_bf16_error/{name}']
        assert bool(torch.isfinite(got.float()).all())
        err = rel_fro(got.float().cpu(), want)
        print(f'[position-train] {kind} {name:44s} error {err:.4f}  bar {bar:.4f}  ({err / bar:.2f})')
        assert err <= bar, name
    assert (NORM[0] in grads) == (kind == 'esm1b')


def test_the_trainable_embedding_is_the_inference_embedding(tmp_path):
    from esme import autograd as ag
    model = _model(tmp_path, 'esm1v').mark_trainable(False, False, positions=True)
    tokens_in, _, _, cu, ml = _batch()
    pe = model.embed_positions
    x = ag.PositionEmbedding.apply(model.embed_tokens.weight, pe.weight, tokens_in, cu, ml, model.alphabet.mask_idx, pe.padding_idx + 1)
    assert x.grad_fn is not None and bool((tokens_in == model.alphabet.mask_idx).any())
    want = model._embedding_phys(tokens_in, (cu, ml))
    assert torch.equal(x.detach().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize('kind', KINDS)
def test_padded_tokens_checkpointing_and_two_runs_give_the_same_bits(tmp_path, kind):
    g = _golden()
    model = _model(tmp_path, kind).mark_trainable(embedding=True, positions=True).train()
    loss = _step(model)
    packed = _grads(model)
    assert torch.equal(_step(model), loss)                                   # two backward runs
    again = _grads(model)
    assert set(again) == set(packed) and all(torch.equal(again[n], packed[n]) for n in packed)
    assert torch.equal(_step(model, checkpoint_layers=True), loss)           # layer checkpointing
    ckpt = _grads(model)
    assert set(ckpt) == set(packed) and all(torch.equal(ckpt[n], packed[n]) for n in packed)
    cu, S = g['cu_lens'].tolist(), int(g['max_len'])                         # 2-D tokens with right padding
    B, pad = len(cu) - 1, model.alphabet.padding_idx
    tok2, in2, mask2 = torch.full((B, S), pad), torch.full((B, S), pad), torch.zeros(B, S, dtype=torch.bool)
    for b, (a, e) in enumerate(zip(cu[:-1], cu[1:])):
        tok2[b, :e - a], in2[b, :e - a], mask2[b, :e - a] = g['esm2_tokens'][a:e], g['esm2_tokens_in'][a:e], g['esm2_mask'][a:e]
    assert bool((in2 == pad).any())
    model.zero_grad(set_to_none=True)
    logits = model.forward_trainable(in2.to(DEV))
    assert logits.shape == (B, S, model.vocab_size)
    esme.cross_entropy(logits, tok2.to(DEV), mask2.to(DEV), alphabet=model.alphabet).backward()
    padded = _grads(model)
    assert set(padded) == set(packed)
    worst = max(rel_fro(padded[n].float(), packed[n].float()) for n in packed)
    print(f'\n[position-train] {kind} 2-D tokens against packed: worst relative difference {worst:.2e}; '
          f'position table {rel_fro(padded[POS].float(), packed[POS].float()):.2e}')
    assert torch.equal(padded[POS], packed[POS])                             # the same packed rows reach the same kernel
    assert worst <= 2.0 ** -8                                                # (the LM head's torch GEMM sums over another row count: test_mlm_train_gpu.py)


@pytest.mark.parametrize('kind', KINDS)
def test_frozen_positions_with_lora_and_the_table_alone(tmp_path, kind):
    model = _model(tmp_path, kind)
    model.mark_trainable(False, False, positions=True).train()               # the table alone: the run that made the 4 096-position checkpoints
    _step(model)
    alone = _grads(model)
    assert set(alone) == {POS} and bool(alone[POS].any())
    with_all = _model(tmp_path, kind).mark_trainable(positions=True).train()
    _step(with_all)
    assert torch.equal(with_all.embed_positions.weight.grad, alone[POS])     # the same d_x whatever else trains
    model.mark_trainable(False, False)                                       # the opt-in withdrawn: refused again, by name
    with pytest.raises(NotImplementedError, match='learned-position'):
        _step(model)
    model.add_lora(rank=4, alpha=8, layers=('query', 'value'))
    model.mark_trainable(False, False, positions='frozen')
    model.mark_only_lora_as_trainable()
    from test_lora_gpu import fill_b
    fill_b(model, 3)
    loss = _step(model)
    grads = _grads(model)
    assert bool(torch.isfinite(loss)) and grads and all('lora_' in n for n in grads) and all(bool(v.any()) for v in grads.values())
    assert model.embed_positions.weight.grad is None and not model.embed_positions.weight.requires_grad
    rep = model.forward_trainable(*_batch()[:1], _batch()[3:], logits=False, layers=[0])       # taps and logits=False as for ESM-2
    assert rep.shape == (_batch()[0].numel(), 2 * model.embed_dim) and rep.grad_fn is not None


def test_regression_model_on_esm1v(tmp_path):
    from esme.trainer import RegressionModel
    model = _model(tmp_path, 'esm1v').mark_trainable(layers=[-1], positions='frozen')
    tokens_in, _, _, cu, ml = _batch()
    head = torch.nn.Linear(2 * model.embed_dim, 1, dtype=torch.bfloat16)
    reg = RegressionModel(model, head, layers=[0], reduction='mean').to(DEV).train()
    cul = cu.tolist()
    pad_indices = torch.cat([b * ml + torch.arange(e - a) for b, (a, e) in enumerate(zip(cul[:-1], cul[1:]))]).to(DEV)
    y = reg.forward_trainable(tokens_in, (cu, ml), pad_output=True, pad_indices=pad_indices)
    assert y.shape == (cu.numel() - 1, 1) and y.grad_fn is not None
    y.float().pow(2).mean().backward()
    assert model.embed_positions.weight.grad is None and bool(head.weight.grad.any())
    assert any(p.grad is not None and bool(p.grad.any()) for n, p in model.named_parameters() if n.startswith(f'layers.{len(model.layers) - 1}.'))


def test_ten_adamw_steps_lower_the_loss(tmp_path):
    model = _model(tmp_path, 'esm1v').mark_trainable(False, False, positions=True).train()
    w = model.embed_positions.weight
    before = w.detach().clone()
    opt = esme.optim.AdamW([w], lr=2e-3, weight_decay=0.0)
    tokens_in, tokens, mask, cu, ml = _batch()
    losses = []
    for step in range(10):
        model.zero_grad(set_to_none=True)
        loss = esme.cross_entropy(model.forward_trainable(tokens_in, (cu, ml)), tokens, mask, alphabet=model.alphabet)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = [float(v) for v in losses]
    print(f'\n[position-train] ten AdamW steps on the position table alone at lr 2e-3: {losses[0]:.4f} -> {losses[-1]:.4f}')
    assert losses[-1] < losses[0] and opt.state[w]['step'] == 10
    rows = ml + 2
    assert not torch.equal(w.detach()[2:rows], before[2:rows]) and torch.equal(w.detach()[rows:], before[rows:]) and torch.equal(w.detach()[:2], before[:2])


def test_forward_and_backward_do_not_synchronise(tmp_path):
    """The position-only set-up under torch's sync debug mode: the lookup, the layers and both backward passes enqueue and return.  The
    loss selects the masked rows through ignore_index (a boolean index would read its row count on the host)."""
    model = _model(tmp_path, 'esm1v').mark_trainable(False, False, positions=True).train()
    tokens_in, tokens, mask, cu, ml = _batch()
    target = torch.where(mask, tokens, torch.full_like(tokens, model.alphabet.padding_idx))

    def step():
        model.zero_grad(set_to_none=True)
        logits = model.forward_trainable(tokens_in, (cu, ml))
        torch.nn.functional.cross_entropy(logits.float(), target, ignore_index=model.alphabet.padding_idx).backward()
    step()                                                                   # (the first step builds derived weights and kernel attributes)
    want = model.embed_positions.weight.grad.clone()
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert torch.equal(model.embed_positions.weight.grad, want) and bool(want.any())


def test_extend_positions_trains_the_new_rows_and_reaches_inference(tmp_path):
    from esme import synthetic as syn
    model = _model(tmp_path, 'esm1v')
    old = model.embed_positions.max_positions
    lengths = [old + 40, 30]                                                 # one sequence longer than the old table serves
    tokens, cu, ml = syn.random_tokens(lengths, 4).to(DEV), syn.cu_lens_of(lengths).to(DEV), max(lengths)
    short = (syn.random_tokens([30, 12], 5).to(DEV), (syn.cu_lens_of([30, 12]).to(DEV), 30))
    model.eval()
    graphed_before = model.graphed(*short)
    assert len(model._graph_cache.entries) == 1
    model.mark_trainable(False, False, positions=True).train()
    with pytest.raises(ValueError, match='above maximum'):                   # refused before any launch, as the inference forward refuses it
        model.forward_trainable(tokens, (cu, ml))
    table = model.embed_positions.weight.detach().clone()
    assert model.extend_positions(2 * old) is model
    w = model.embed_positions.weight
    assert w.shape[0] == 2 * old + 2 and w.requires_grad and w.is_cuda and torch.equal(w.detach()[:old + 2], table) and not bool(w.detach()[old + 2:].any())
    assert len(model._graph_cache.entries) == 0                              # the graph captured with the old table is gone
    logits = model.forward_trainable(tokens, (cu, ml))
    logits.float().logsumexp(-1).mean().backward()
    grad = w.grad
    assert grad.shape == w.shape and bool(grad[old + 2:ml + 2].any(dim=1).all()) and not bool(grad[ml + 2:].any())      # the gradient reaches the new rows
    with torch.no_grad():
        w[2:] += 0.5                                                         # the table changes, new rows included
    model.eval()
    out = model(tokens, (cu, ml))                                            # the inference forward reads the extended table
    assert out.shape[0] == tokens.numel() and bool(torch.isfinite(out.float()).all())
    with torch.no_grad():
        w[old + 2:] -= 0.5
    assert not torch.equal(model(tokens, (cu, ml))[old + 2:old + 40], out[old + 2:old + 40])               # ... its new rows too
    model.invalidate_graphs()
    graphed_after = model.graphed(*short)                                    # captured anew, on the table as it is now
    assert torch.equal(graphed_after, model(*short)) and not torch.equal(graphed_after, graphed_before)
