"""Adapters over a quantised base on the device (add_lora(quantized_base=True)): the tiny synthetic checkpoints of the LoRA tests (ESM-2: 2
layers, E = 128, 4 heads, d = 32; ESM-C: 2 layers, E = 128, 2 heads, d = 64) loaded in '4bit' and '8bit', one packed batch of lengths 5, 9, 64, 65.

The numerical criterion is bit-equality with the TWIN: the same checkpoint loaded in bfloat16, every projection weight overwritten with
the quantised model's lin.dequantize(), the same adapters copied in.  Both run the same GEMM kernel on operands that hold the same bits
(the expansion of W in the forward, the transposing expansion of W^T in the backward against the twin's cached W^T), so logits, loss
and every gradient must be torch.equal; the twin's own path is held to float64 autograd by tests/test_lora_train_gpu.py.  Then: nothing
of weight size is kept, peak memory against the twin, a training run that saves and reloads, the fused inference forward with the
extension block next to the per-call expansion (bit-identical with fresh adapters, within the per-element bounds of the extended GEMMs
on the operands handed to them once trained, and at the floor between the fused and the unfused pipelines against forward_trainable),
and the refusals that stay."""
import gc

import pytest
import torch

import error_bounds as eb
import esme
import lora_bounds as lb
from esme import ESM, _hip, synthetic as syn
from golden_util import rel_fro
from test_lora_gpu import fill_b, tiny

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LENGTHS = [5, 9, 64, 65]
GEOMETRY = {'esm2': (2, 128, 4), 'esmc': (2, 128, 2)}
CASES = [(kind, quant) for kind in GEOMETRY for quant in ('4bit', '8bit')]
LORA = dict(rank=8, alpha=16, layers=('query', 'key', 'value', 'output'))
FLOOR = 2.5e-2          # between the fused and the unfused bf16 pipelines: the bar of tests/test_full_train_gpu.py::test_ten_adamw_steps_reach_the_inference_forward


def _path(tmp_path, kind, L, E, H, seed=3):
    return syn.write_checkpoint(str(tmp_path / f'{kind}_{L}_{E}_{H}_{seed}_q.safetensors'), f'{kind}_t', L, E, H, seed=seed)


def _quantised(tmp_path, kind, quant, geometry=None):
    return ESM.from_pretrained(_path(tmp_path, kind, *(geometry or GEOMETRY[kind])), quantization=quant, device=DEV)


def _projections(model):
    """(name, module) of every layer's own projections, adapters unwrapped."""
    from esme.lora import LoRA
    out = []
    for i, layer in enumerate(model.layers):
        att = layer.self_attn
        mods = [(f'self_attn.{p}', getattr(att, p)) for p in ('q', 'k', 'v', 'out')]
        if layer.final_activation == 'gelu':
            mods += [('final.1', layer.final[1]), ('final.3', layer.final[3])]
        else:
            mods += [('final.1.activation', layer.final[1].activation), ('final.1.fc', layer.final[1].fc), ('final.2', layer.final[2])]
        out += [(f'layers.{i}.{n}', m.layer if isinstance(m, LoRA) else m) for n, m in mods]
    return out


def _twin(tmp_path, kind, q, geometry=None):
    """The bfloat16 model that holds the quantised model's expanded weights, with its adapters (if any)."""
    twin = ESM.from_pretrained(_path(tmp_path, kind, *(geometry or GEOMETRY[kind])), device=DEV)
    with torch.no_grad():
        for (n, a), (m, b) in zip(_projections(twin), _projections(q)):
            assert n == m and a.weight.dtype == torch.bfloat16
            a.weight.data.copy_(b.dequantize())
            assert (a.bias is None) == (b.bias is None) and (a.bias is None or torch.equal(a.bias, b.bias))
    twin.invalidate_graphs()
    if q.has_lora:
        twin.add_lora(**LORA)
        own = dict(twin.named_parameters())
        with torch.no_grad():
            for n, p in q.named_parameters():
                if '.lora_' in n:
                    own[n].copy_(p)
    return twin


def _adapted(tmp_path, kind, quant, seed=1, b_scale=0.1):
    torch.manual_seed(seed)
    q = _quantised(tmp_path, kind, quant).add_lora(**LORA, quantized_base=True)
    if b_scale:
        fill_b(q, seed, b_scale)
    return q


def _batch(model, lengths=LENGTHS, seed=2):
    tokens = syn.random_tokens(lengths, seed)
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(tokens.shape, generator=g) < 0.3
    tokens_in = torch.where(mask, torch.full_like(tokens, model.alphabet.mask_idx), tokens)
    return tokens_in.to(DEV), tokens.to(DEV), mask.to(DEV), (syn.cu_lens_of(lengths).to(DEV), max(lengths))


def _step(model, batch, **kw):
    tokens_in, tokens, mask, pad_args = batch
    model.zero_grad(set_to_none=True)
    logits = model.forward_trainable(tokens_in, pad_args, **kw)
    assert logits.grad_fn is not None and logits.dtype == torch.bfloat16
    loss = esme.cross_entropy(logits, tokens, mask, alphabet=model.alphabet)
    loss.backward()
    return logits.detach(), loss.detach()


def _grads(model):
    return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


# ------------------------------------------------------------------ 1. bit-equality with the twin

@pytest.mark.parametrize('kind,quant', CASES)
def test_training_step_is_bit_equal_to_the_twin(tmp_path, kind, quant):
    q = _adapted(tmp_path, kind, quant).mark_lmhead(True).train()
    twin = _twin(tmp_path, kind, q).mark_lmhead(True).train()
    batch = _batch(q)
    for kw in ({}, {'checkpoint_layers': True}):
        lq, loss_q = _step(q, batch, **kw)
        gq = _grads(q)
        lt, loss_t = _step(twin, batch, **kw)
        gt = _grads(twin)
        print(f'\n[qlora] {kind} {quant} {kw or "plain"}: loss {float(loss_q):.6f} (twin {float(loss_t):.6f}), {len(gq)} gradients')
        assert torch.equal(lq, lt) and torch.equal(loss_q, loss_t)
        assert set(gq) == set(gt) and any('.lora_A.' in n for n in gq) and any(n.startswith('lm_head.') for n in gq)
        assert all('.lora_' in n or n.startswith('lm_head.') for n in gq)
        for n in gq:
            assert bool(gq[n].any()), f'{n}: zero gradient'
            assert torch.equal(gq[n], gt[n]), f'{kind} {quant} {kw}: gradient of {n} differs from the twin'


def test_nf4_codebook_trains_bit_equal_to_its_twin(tmp_path):
    from esme.quantization import quantize_model_
    kind = 'esm2'
    torch.manual_seed(1)
    q = quantize_model_(tiny(tmp_path, kind, *GEOMETRY[kind], 3), 'nf4').add_lora(**LORA, quantized_base=True)
    assert q.quantization == '4bit-nf4' and q.layers[0].self_attn.q.layer.quant_type == 'nf4'
    fill_b(q, 1)
    twin = _twin(tmp_path, kind, q)
    batch = _batch(q)
    (lq, loss_q), (lt, loss_t) = _step(q.train(), batch), _step(twin.train(), batch)
    assert torch.equal(lq, lt) and torch.equal(loss_q, loss_t)
    gq, gt = _grads(q), _grads(twin)
    assert set(gq) == set(gt) and all(torch.equal(gq[n], gt[n]) for n in gq)


# ------------------------------------------------------------------ 2. nothing of weight size is kept

@pytest.mark.parametrize('kind,quant', CASES)
def test_nothing_of_weight_size_is_kept(tmp_path, kind, quant):
    q = _adapted(tmp_path, kind, quant).train()
    codes = {n: (m.weight.data.clone(), m.absmax.clone()) for n, m in _projections(q)}
    batch = _batch(q)
    _step(q, batch)
    _step(q, batch, checkpoint_layers=True)
    for layer in q.layers:
        for holder in (layer, layer.self_attn, *( [layer.final[1]] if layer.final_activation != 'gelu' else [])):
            assert holder._derived.key('wt') is None, 'a transposed weight was cached'
            assert not [t for t in holder._derived.tensors() if t.numel() >= 128 * 128], 'a weight-sized derived tensor was cached'
    for n, m in _projections(q):
        assert getattr(m, '_derived', None) is None or m._derived.key('wt') is None, n
        assert torch.equal(m.weight.data, codes[n][0]) and torch.equal(m.absmax, codes[n][1]), f'{n}: the codes changed'
        assert not m.weight.requires_grad and m.weight.grad is None and not m.absmax.requires_grad
    largest = max(m.out_features * m.in_features for _, m in _projections(q))
    assert q._q4_scratch.buf.numel() == largest, (q._q4_scratch.buf.numel(), largest)
    # once the fused forward has run: the largest packed matrix of the inference path, the adapters' extension columns included
    q.eval()
    q(batch[0], batch[3])
    X_qkv, X_out = q.layers[0].self_attn.lora_ext_widths(None)
    assert X_qkv == 64 and X_out == 64
    packed = []
    for layer in q.layers:
        att = layer.self_attn
        packed += [att._q4_qkv.rows * (att._q4_qkv.cols + X_qkv), att._q4_out.rows * (att._q4_out.cols + X_out),
                   layer._q4_up.rows * layer._q4_up.cols, layer._q4_down.rows * layer._q4_down.cols]
    assert q._q4_scratch.buf.numel() == max(largest, *packed), (q._q4_scratch.buf.numel(), largest, packed)
    cached = list(q.layers[0].self_attn._derived.tensors())
    assert cached and max(t.numel() for t in cached) <= 3 * 128 * 64, 'the adapter cache holds more than the extension blocks'


# ------------------------------------------------------------------ 3. peak memory against the twin

def test_peak_memory_is_lower_than_the_twins(tmp_path):
    """2 layers, E = 640, 20 heads: the weights dominate the 64-row batch.  Each model is measured alone on the device.  The bound, 2 bytes
    per projection weight, is the twin's cached transposed copies alone; the codes against the bfloat16 weights give more."""
    kind, geometry = 'esm2', (2, 640, 20)

    def peak(model):
        batch = _batch(model, [30, 34])
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        _step(model.train(), batch)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated()

    def fresh():
        torch.manual_seed(1)
        return _quantised(tmp_path, kind, '4bit', geometry).add_lora(**LORA, quantized_base=True)

    q = fresh()
    weights = sum(m.out_features * m.in_features for _, m in _projections(q))
    twin = _twin(tmp_path, kind, q, geometry)
    del q
    gc.collect()
    torch.cuda.empty_cache()
    peak_twin = peak(twin)
    del twin
    gc.collect()
    torch.cuda.empty_cache()
    peak_q = peak(fresh())
    print(f'\n[qlora] peak memory of one forward + backward, E = 640, 64 rows: quantised base {peak_q} B, bfloat16 twin {peak_twin} B; '
          f'difference {peak_twin - peak_q} B = {(peak_twin - peak_q) / weights:.2f} B per projection weight ({weights} weights)')
    assert peak_twin - peak_q >= 2 * weights


# ------------------------------------------------------------------ 4. a training run; 5. the fused inference forward

def _train(q, batch, steps=10):
    opt = esme.optim.AdamW([p for p in q.parameters() if p.requires_grad], lr=5e-3, weight_decay=0.0)
    losses = []
    q.train()
    for _ in range(steps):
        losses.append(float(_step(q, batch)[1]))
        opt.step()
    return losses


@pytest.mark.parametrize('kind,quant', CASES)
def test_ten_adamw_steps_save_load_and_the_fused_forward(tmp_path, kind, quant):
    q = _adapted(tmp_path, kind, quant, b_scale=0)
    batch = _batch(q)
    tokens, pad_args = batch[1], batch[3]
    q.eval()
    before = q(tokens, pad_args).clone()
    losses = _train(q, batch)
    print(f'\n[qlora] {kind} {quant} ten esme.optim.AdamW steps: loss ' + ' '.join(f'{v:.4f}' for v in losses))
    assert losses[-1] < losses[0], losses
    trained = q.forward_trainable(tokens, pad_args).detach()
    path = str(tmp_path / 'qlora.safetensors')
    q.save_lora(path)
    fresh = _quantised(tmp_path, kind, quant)
    with pytest.raises(NotImplementedError, match='quanti'):
        fresh.load_lora(path)
    assert not fresh.has_lora
    fresh.load_lora(path, quantized_base=True)
    assert torch.equal(fresh.forward_trainable(tokens, pad_args).detach(), trained)
    # the fused inference forward runs the trained adapters
    q.eval()
    after = q(tokens, pad_args)
    assert not torch.equal(after, before) and torch.equal(fresh.eval()(tokens, pad_args), after)
    e = rel_fro(after.float().cpu(), trained.float().cpu())
    print(f'[qlora] {kind} {quant} model(...) against forward_trainable after the steps: {e:.3e} (floor {FLOOR})')
    assert e <= FLOOR
    rep = q.forward_representation(tokens, pad_args, layers=[0])
    assert torch.equal(q.lm_head(rep[:, :q.embed_dim].contiguous()), after)
    assert torch.equal(q.predict_log_prob(tokens, pad_args), fresh.predict_log_prob(tokens, pad_args))


@pytest.mark.parametrize('kind,quant', CASES)
def test_fresh_adapters_change_no_bit_of_the_quantised_forward(tmp_path, kind, quant):
    base = _quantised(tmp_path, kind, quant)
    q = _adapted(tmp_path, kind, quant, b_scale=0)
    tokens_in, tokens, _, pad_args = _batch(q)
    assert torch.equal(q(tokens, pad_args), base(tokens, pad_args))                       # the LayerNorm-folded form
    x0 = base.embedding(tokens, pad_args)
    with _hip.stream_scope(DEV):                                                           # the unfused stage form
        ctx_q, ctx_b = (m._context(pad_args[0], pad_args[1], x0.shape[0], x0.device) for m in (q, base))
        assert torch.equal(q.layers[0].self_attn(x0, *pad_args, None, ctx_q), base.layers[0].self_attn(x0, *pad_args, None, ctx_b))
    fill_b(q, 1)
    assert not torch.equal(q(tokens, pad_args), base(tokens, pad_args))


@pytest.mark.parametrize('kind,quant', CASES)
def test_extended_gemms_on_the_expanded_image_are_within_their_bounds(tmp_path, kind, quant):
    """Layer 0 of a trained model: the LayerNorm-folded QKV GEMM over [x | u] and the out-projection over [a | u], each judged per
    element against float64 on the operands handed to it -- W is the image in the weight scratch (the per-call expansion next to the
    cached extension block) -- and their down-projections u within lora_bounds.down_reference."""
    q = _adapted(tmp_path, kind, quant, b_scale=0)
    batch = _batch(q)
    _train(q, batch, steps=4)
    q.eval()
    tokens, pad_args = batch[1], batch[3]
    att = q.layers[0].self_attn
    E, eps = q.embed_dim, att.norm.eps
    x0 = q.embedding(tokens, pad_args)
    with _hip.stream_scope(DEV):
        sums = _hip.row_sums(x0)
        lw = att._lora_weights(None, True)
        X, Ap, c1A, bA, block = lw['qkv']
        R = 3 * LORA['rank']
        assert X == 64 and Ap.shape == (R, E) and block.block.shape == (3 * E, X) and not bool(block.block[:, R:].any())
        xe, we, c1, c2 = att._qkv_operands(x0, sums, None, lw, False, None)
        we = we.clone()                                                                   # (the scratch is overwritten by the next expansion)
        assert torch.equal(we[:, :E], att._q4_qkv.folded()[0]) and torch.equal(we[:, E:], block.block)
        qkv = _hip.gemm_fused(xe, we, None, ln=(sums, E, eps, c1, c2, None))
        u_ref, u_bound, _ = lb.down_reference(x0.cpu(), Ap.cpu(), sums.cpu(), E, eps, c1A.cpu(), bA.cpu())
        w_u = eb.assert_bounded(xe[:, E:E + R].cpu(), u_ref, u_bound, f'{kind} {quant} QKV down-projection')
        y, pre = eb.ln_fold_reference(xe.cpu(), we.cpu(), c1.cpu(), c2.cpu(), eps, sums=sums.cpu(), dim=E)
        w_qkv = eb.assert_bounded(qkv.cpu(), y, pre + eb.out_round(y, pre, 'bf16'), f'{kind} {quant} extended QKV GEMM')
        delta = float((xe[:, E:].double() @ we[:, E:].double().T).abs().max())
        assert delta > 0, 'the trained adapters contribute nothing'
        # the out-projection, on the attention output of the unfused stages
        qh, kh, vh = att._qkv(x0, None)
        Xo, Ao, oblock = att._lora_weights(None, True)['out']
        ae, wo, bo = att._out_operands(lw, False, qh, kh, vh, *pad_args)
        wo = wo.clone()
        assert torch.equal(wo[:, :E], att.out.layer.dequantize()) and torch.equal(wo[:, E:], oblock.block)
        alpha = 1.0 / q.layers[0].residue_scaling
        out = _hip.gemm_fused(ae, wo, bo, _hip.EPI_RESIDUAL, x0, alpha)
        ref, bound, _ = eb.gemm_reference(ae.cpu(), wo.cpu(), bo.cpu() if bo is not None else None, 'residual', x0.cpu(), alpha)
        w_out = eb.assert_bounded(out.cpu(), ref, bound, f'{kind} {quant} extended out-projection')
        uo_ref, uo_bound, _ = lb.down_reference(ae[:, :E].cpu(), Ao.cpu())
        eb.assert_bounded(ae[:, E:E + LORA['rank']].cpu(), uo_ref, uo_bound, 'its down-projection')
    print(f'\n[qlora] {kind} {quant} layer 0 on the expanded image: worst err / bound QKV {w_qkv:.3f} (its u {w_u:.3f}), out-projection {w_out:.3f}; '
          f'largest adapter term {delta:.3e}')


def test_adapter_selection_reproduces_the_bits_and_refusals_stay(tmp_path):
    kind = 'esm2'
    torch.manual_seed(4)
    q = _quantised(tmp_path, kind, '4bit').add_lora(rank=5, alpha=7, adapter_names=['a', 'b'], quantized_base=True)
    fill_b(q, 3, scale=1.0)
    tokens_in, tokens, _, pad_args = _batch(q)
    a1 = q(tokens, pad_args, lora_names=['a'])
    b1 = q(tokens, pad_args, lora_names=['b'])
    a2 = q(tokens, pad_args, lora_names=['a'])
    assert torch.equal(a1, a2) and not torch.equal(a1, b1)
    assert torch.equal(q(tokens, pad_args), q(tokens, pad_args, lora_names=['a', 'b']))
    # 6. refusals on the device
    with pytest.raises(NotImplementedError, match='graph'):
        q.graphed(tokens, pad_args)
    with pytest.raises(NotImplementedError, match='quantised'):
        q.mark_trainable()
    with pytest.raises(NotImplementedError, match='quanti'):
        _quantised(tmp_path, kind, '4bit').add_lora()
    plain = _quantised(tmp_path, kind, '8bit')
    with pytest.raises(NotImplementedError, match='quantised'):
        plain.forward_trainable(tokens_in, pad_args)
    q.layers[1].final[0].weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match=r'final\.0\.weight'):
        q.forward_trainable(tokens_in, pad_args)
    q.layers[1].final[0].weight.requires_grad_(False)
    q.train()
    with pytest.raises(NotImplementedError, match='inference only'):
        q(tokens, pad_args)
