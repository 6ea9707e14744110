"""LoRA adapters on the FFN projections on the device (ESM2.add_lora(layers=(..., 'ffn_up', 'ffn_down'))): tiny ESM-2 (2 layers, E = 128,
2 heads, GELU, F = 512) and tiny ESM-C (the same geometry, SwiGLU, q / k LayerNorm), one packed batch of the lengths 1, 63, 64, 65, 127,
128, 129 (the GEMM's tile edge, the 128-row workgroup edge of esme_hip_lora_down; T = 577).

 1. fresh adapters (every lora_B zero) on all six targets change no bit, LayerNorm-folded and unfused;
 2. esme_hip_lora_down at K = F = 512 followed by the residual GEMM over K = F + X, per element against float64 on the operands handed to
    them (tests/lora_bounds.py::down_reference and tests/error_bounds.py::gemm_reference serve any K: nothing is restated);
 3. the fused FFN branch of one layer against a float64 restatement, with the adapter-free layer's error measured in the same run;
 4. model(...) against forward_trainable(...);
 5. the gradients of the FFN adapters against float64 autograd of a restatement of the whole model;
 6. selecting one adapter of three equals a model that holds only that one, bit for bit;
 7. QLoRA: the fused forward against the bfloat16 twin that holds the expanded weights, a training step, nothing of weight size kept.
A run's figures are kept in profiles/lora_ffn_parity.txt."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import error_bounds as eb
import esme
import lora_bounds as lb
from esme import ESM, _hip, synthetic as syn
from esme.lora import LoRA
from golden_util import rel_fro
from oracle import esm_oracle as O
from test_lora_gpu import fill_b, rnd, tiny
from test_qlora_gpu import _projections

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KINDS = ('esm2', 'esmc')
L, E, H, FF = 2, 128, 2, 512
LENGTHS = (1, 63, 64, 65, 127, 128, 129)
ALL_SIX = ('query', 'key', 'value', 'output', 'ffn_up', 'ffn_down')
SEED = 9


def batch(seed=5):
    return syn.random_tokens(list(LENGTHS), seed).to(DEV), (syn.cu_lens_of(list(LENGTHS)).to(DEV), max(LENGTHS))


def masked_batch(model, seed=2):
    tokens = syn.random_tokens(list(LENGTHS), seed)
    mask = torch.rand(tokens.shape, generator=torch.Generator().manual_seed(seed)) < 0.3
    tokens_in = torch.where(mask, torch.full_like(tokens, model.alphabet.mask_idx), tokens)
    return tokens_in.to(DEV), tokens.to(DEV), mask.to(DEV), (syn.cu_lens_of(list(LENGTHS)).to(DEV), max(LENGTHS))


def adapted(tmp_path, kind, layers=ALL_SIX, names=('a', 'b'), rank=16, alpha=24, b_seed=1, b_scale=0.1):
    torch.manual_seed(3)
    model = tiny(tmp_path, kind, L, E, H, SEED).add_lora(rank=rank, alpha=alpha, layers=layers, adapter_names=list(names))
    if b_scale:
        fill_b(model, b_seed, b_scale)
    return model


# ------------------------------------------------------------------ 1. zero B

@pytest.mark.parametrize('kind', KINDS)
def test_fresh_ffn_adapters_change_no_bit(kind, tmp_path):
    tokens, pad_args = batch()
    base = tiny(tmp_path, kind, L, E, H, SEED)
    want = base(tokens, pad_args)
    rep = base.forward_representation(tokens, pad_args, layers=[0, 1])
    model = adapted(tmp_path, kind, b_scale=0)
    layer = model.layers[0]
    assert layer.ffn_lora_ext_widths(None) == (64, 64) and layer.self_attn.lora_ext_widths(None) == (128, 64)      # (SwiGLU's up GEMM: 2 x 2 x 16 = 64 rows)
    assert layer.ffn_lora_ext_widths(['a']) == (64, 64) and model.layers[1].self_attn.lora_ext_widths(['a']) == (64, 64)
    assert torch.equal(model(tokens, pad_args), want)
    assert torch.equal(model(tokens, pad_args, lora_names=['b']), want)
    assert torch.equal(model.forward_representation(tokens, pad_args, layers=[0, 1]), rep)
    only_ffn = adapted(tmp_path, kind, layers=('ffn_up', 'ffn_down'), b_scale=0)       # (no QKV adapter: the stream buffer is there for the FFN alone)
    assert torch.equal(only_ffn(tokens, pad_args), want)
    only_down = adapted(tmp_path, kind, layers=('ffn_down',), b_scale=0)                # (no stream buffer at all)
    assert torch.equal(only_down(tokens, pad_args), want)
    base.fold_layernorm = model.fold_layernorm = False                                  # the unfused form: LayerNorm kernel, plain GEMMs
    assert torch.equal(model(tokens, pad_args), base(tokens, pad_args))
    base.fold_layernorm = model.fold_layernorm = True
    fill_b(model, 1)
    assert not torch.equal(model(tokens, pad_args), want)
    for name in ('final.1.fc' if kind == 'esmc' else 'final.1', 'final.2' if kind == 'esmc' else 'final.3'):      # each FFN adapter alone reaches the output
        fill_b(only_ffn, 1, 0.0)
        with torch.no_grad():
            p = dict(only_ffn.named_parameters())[f'layers.1.{name}.lora_B.a']
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(4)).to(p.dtype) * 0.05)
        assert not torch.equal(only_ffn(tokens, pad_args), want), name


# ------------------------------------------------------------------ 2. the kernel at K = F and the residual GEMM over K = F + X

@pytest.mark.parametrize('X,R', [(64, 4), (64, 20), (128, 4), (128, 20)])
def test_lora_down_at_ffn_width_and_extended_residual_gemm_vs_float64(X, R):
    K, N, T = FF, E, sum(LENGTHS)
    rng = np.random.Generator(np.random.PCG64(K + X + R))
    mid = torch.full((T, K + X), 7.0, dtype=torch.bfloat16, device=DEV)                # as the up GEMM leaves it: the activation in the first K columns
    act = (rnd(rng, T, K).float() * (0.5 + rnd(rng, 1, K).float().abs())).bfloat16().to(DEV)
    mid[:, :K] = act
    A = rnd(rng, R, K, scale=K ** -0.5).to(DEV)
    _hip.lora_down(mid[:, :K], A, mid[:, K:])
    torch.cuda.synchronize()
    assert torch.equal(mid[:, :K], act) and not bool(mid[:, K + R:].any()), 'the activation is left as it was; columns past the ranks are zero'
    u_ref, u_bound, _ = lb.down_reference(act.cpu(), A.cpu())
    w_u = eb.assert_bounded(mid[:, K:K + R].cpu(), u_ref, u_bound, f'lora_down K={K} X={X} R={R}')
    W, bias, resid = rnd(rng, N, K, scale=K ** -0.5).to(DEV), rnd(rng, N, scale=0.1).to(DEV), rnd(rng, T, N).to(DEV)
    we = torch.zeros(N, K + X, dtype=torch.bfloat16, device=DEV)
    we[:, :K], we[:, K:K + R] = W, rnd(rng, N, R, scale=0.3 * R ** -0.5).to(DEV)
    stats = torch.empty(_hip.stats_blocks(T, N), T, 2, dtype=torch.float32, device=DEV)
    out = _hip.gemm_fused(mid, we, bias, _hip.EPI_RESIDUAL, resid, 0.75, stats_out=stats)
    ref, bound, _ = eb.gemm_reference(mid.cpu(), we.cpu(), bias.cpu(), 'residual', resid.cpu(), 0.75)
    w_o = eb.assert_bounded(out.cpu(), ref, bound, f'residual GEMM over K = {K} + {X}')
    delta = (u_ref @ we[:, K:K + R].double().cpu().T).abs() * 0.75
    print(f'\n[lora-ffn] K={K} X={X} R={R} T={T}: worst err / bound lora_down {w_u:.3f}, residual GEMM {w_o:.3f}; median |delta| / bound {float((delta / bound).median()):.1f}')
    s, o = stats.sum(0).double().cpu(), out.double().cpu()
    assert torch.allclose(s[:, 0], o.sum(1), rtol=1e-4, atol=1e-3) and torch.allclose(s[:, 1], (o * o).sum(1), rtol=1e-4, atol=1e-3)


# ------------------------------------------------------------------ 3. the fused branch against float64

@torch.no_grad()
def ffn_branch64(layer, x, adapters=True):
    """LayerNorm -> up + adapters -> GELU, or silu(g) * f -> down + adapters, over the residue scaling, in float64 on the layer's bf16 parameters."""
    ln = layer.final[0]
    h = F.layer_norm(x.double(), (x.shape[1],), ln.weight.double(), ln.bias.double() if ln.bias is not None else None, ln.eps)

    def lin(m, v):
        base = m.layer if isinstance(m, LoRA) else m
        y = F.linear(v, base.weight.double(), base.bias.double() if base.bias is not None else None)
        if adapters and isinstance(m, LoRA):
            for n in m.select(None):
                y = y + F.linear(F.linear(v, m.lora_A[n].double()), m.lora_B[n].double()) * m.scaling
        return y
    ups, (_, down) = layer._ffn_projections()
    u = F.gelu(lin(ups[0][1], h)) if len(ups) == 1 else F.silu(lin(ups[0][1], h)) * lin(ups[1][1], h)
    return lin(down, u) / layer.residue_scaling


def fused_branch(layer, x, fold):
    with _hip.stream_scope(DEV):
        out = torch.empty_like(x)
        layer._ffn(x, 1.0 / layer.residue_scaling, {'resid': torch.zeros_like(x), 'out': out}, x_stats=_hip.row_sums(x) if fold else None)
    return out


@pytest.mark.parametrize('kind', KINDS)
def test_fused_ffn_branch_vs_float64_restatement(kind, tmp_path):
    """The measure and the ratio are those tests/test_lora_gpu.py holds the models with attention adapters to (its line 189:
    assert_parity, whose first assertion is tests/test_model_gpu.py:47): relative Frobenius error against the exact result, at most
    max(1.25 x the error of the adapter-free pipeline against ITS exact result, 4e-3).  There the adapter-free error is the
    reference's bf16 forward; here it is this layer's own adapter-free branch, measured in the same run."""
    tokens, pad_args = batch()
    base, model = tiny(tmp_path, kind, L, E, H, SEED), adapted(tmp_path, kind)
    x = base.embedding(tokens, pad_args)
    with torch.no_grad():
        x = (x.float() * 3.0 + 0.25).bfloat16()                       # (rows with a mean and a spread: the LayerNorm has something to do)
    failures = []
    for fold in (True, False):
        e_base = rel_fro(fused_branch(base.layers[0], x, fold).double(), ffn_branch64(base.layers[0], x))
        got, ref = fused_branch(model.layers[0], x, fold).double(), ffn_branch64(model.layers[0], x)
        e_lora = rel_fro(got, ref)
        share = rel_fro(ref, ffn_branch64(model.layers[0], x, adapters=False))
        print(f"\n[lora-ffn parity] {kind} FFN branch, {'LayerNorm-folded' if fold else 'unfused'}: adapter-free {e_base:.3e} | all FFN adapters {e_lora:.3e} "
              f'| bar {max(1.25 * e_base, 4e-3):.3e} | adapters move the branch by {share:.2f} of its norm')
        assert share > 0.05, 'the adapters contribute next to nothing: the comparison would show nothing'
        if not e_lora <= max(1.25 * e_base, 4e-3):
            failures.append((fold, e_lora, e_base))
    assert not failures, failures


# ------------------------------------------------------------------ 4. fused against trainable

@pytest.mark.parametrize('kind', KINDS)
def test_model_forward_vs_forward_trainable(kind, tmp_path):
    """tests/test_lora_train_gpu.py::test_forward_trainable_computes_the_inference_forward holds the two pipelines to
    rel_fro <= min(max(2e-2, 1.6 e_ref), 2.5e-2) with e_ref the reference's bf16 error from its fixture; there is no fixture here, so
    the bar is that expression's smallest value, 2e-2."""
    tokens, pad_args = batch()
    model = adapted(tmp_path, kind).eval()
    y = model(tokens, pad_args)
    t = model.forward_trainable(tokens, pad_args)
    assert t.grad_fn is not None and t.shape == y.shape and t.dtype == y.dtype
    e = rel_fro(t.detach().float().cpu(), y.float().cpu())
    base = tiny(tmp_path, kind, L, E, H, SEED)
    moved = rel_fro(y.float().cpu(), base(tokens, pad_args).float().cpu())
    print(f'\n[lora-ffn parity] {kind} model(...) against forward_trainable(...), all six targets: {e:.3e} (bar 2e-2); the adapters move the logits by {moved:.3e}')
    assert moved > 2e-2, 'the adapters move the logits by less than the bar: the comparison would show nothing'
    assert e <= 2e-2
    e_b = rel_fro(model.forward_trainable(tokens, pad_args, lora_names=['b']).detach().float().cpu(), model(tokens, pad_args, lora_names=['b']).float().cpu())
    assert e_b <= 2e-2, e_b


# ------------------------------------------------------------------ 5. gradients

def restated_loss(w, adapters, scaling, tokens_in, tokens, mask, cu, max_len, dtype):
    """The tiny ESM-2 model in torch ops in `dtype` on the weights `w`: the oracle's embedding, attention block and LM head around an FFN
    that carries the adapters {(layer, 'final.1' / 'final.3'): {name: (A, B)}} in the reference's data flow (base + s B (A x))."""
    x = O.embedding(w, tokens_in, 'esm2', dtype, cu)
    for i in range(L):
        x = x + O.attention_block(w, i, x, cu, max_len, H, 'esm2', dtype)
        p = f'layers.{i}.final.'
        h = O._ln(x, w[p + '0.weight'].to(dtype), w[p + '0.bias'].to(dtype))

        def lin(key, v):
            y = F.linear(v, w[p + key + '.weight'].to(dtype), w[p + key + '.bias'].to(dtype))
            for A, B in adapters[(i, 'final.' + key)].values():
                y = y + F.linear(F.linear(v, A), B) * scaling
            return y
        x = x + lin('3', F.gelu(lin('1', h)))
    x = O._ln(x, w['emb_layer_norm_after.weight'].to(dtype), w['emb_layer_norm_after.bias'].to(dtype))
    return esme.cross_entropy(O.lm_head(w, x, dtype), tokens, mask)


def test_ffn_adapter_gradients_vs_float64_autograd(tmp_path):
    """The bar of tests/test_lora_train_gpu.py per tensor -- relative Frobenius error against the float64 gradient at most 2 x the error of
    the reference data flow's own bf16 gradient against its fp32 gradient -- with the three gradients taken from the restatement above
    (there: from the fixture of the reference)."""
    model = adapted(tmp_path, 'esm2', layers=('ffn_up', 'ffn_down'), rank=8, alpha=16).train()
    tokens_in, tokens, mask, (cu, ml) = masked_batch(model)
    model.zero_grad(set_to_none=True)
    loss = esme.cross_entropy(model.forward_trainable(tokens_in, (cu, ml)), tokens, mask, alphabet=model.alphabet)
    loss.backward()
    w = {k.replace('.layer.', '.'): v.detach().cpu() for k, v in model.state_dict().items() if '.lora_' not in k}
    cpu = [t.cpu() for t in (tokens_in, tokens, mask, cu)]
    grads = {}
    for dtype in (torch.float64, torch.float32, torch.bfloat16):
        ad, leaves = {}, {}
        for i, layer in enumerate(model.layers):
            for key in ('final.1', 'final.3'):
                m = layer.final[int(key[-1])]
                ad[(i, key)] = {}
                for n in m.lora_A:
                    A, B = (p.detach().cpu().to(dtype).requires_grad_() for p in (m.lora_A[n], m.lora_B[n]))
                    ad[(i, key)][n] = (A, B)
                    leaves[f'layers.{i}.{key}.lora_A.{n}'], leaves[f'layers.{i}.{key}.lora_B.{n}'] = A, B
        ref_loss = restated_loss(w, ad, model.layers[0].final[1].scaling, *cpu, ml, dtype)
        ref_loss.backward()
        grads[dtype] = ({k: t.grad for k, t in leaves.items()}, float(ref_loss))
    g64, g32, gbf = (grads[d][0] for d in (torch.float64, torch.float32, torch.bfloat16))
    print(f'\n[lora-ffn train] loss {float(loss):.5f}; restatement float64 {grads[torch.float64][1]:.5f}, fp32 {grads[torch.float32][1]:.5f}, bf16 {grads[torch.bfloat16][1]:.5f}')
    failures, seen = [], 0
    for name, p in model.named_parameters():
        if '.lora_' not in name:
            assert p.grad is None and not p.requires_grad, f'{name}: a base weight got a gradient'
            continue
        seen += 1
        assert p.grad is not None and p.grad.dtype == p.dtype and bool(torch.isfinite(p.grad.float()).all()) and bool(p.grad.any()), name
        bar = 2 * rel_fro(gbf[name].float(), g32[name])
        err = rel_fro(p.grad.float().cpu(), g64[name])
        print(f'[lora-ffn train] {name:40s} error {err:.4f}  bar {bar:.4f}  ({err / bar:.2f})')
        if err > bar:
            failures.append((name, err, bar))
    assert seen == len(g64) == L * 2 * 2 * 2
    assert not failures, failures


# ------------------------------------------------------------------ 6. selection

@pytest.mark.parametrize('kind', KINDS)
def test_one_of_three_adapters_equals_a_model_with_that_one(kind, tmp_path):
    tokens, pad_args = batch()
    three = adapted(tmp_path, kind, names=('x', 'y', 'z'), rank=5, alpha=7, b_scale=1.0)
    lone = adapted(tmp_path, kind, names=('y',), rank=5, alpha=7, b_scale=0)
    src = dict(three.named_parameters())
    with torch.no_grad():
        for n, p in lone.named_parameters():
            if '.lora_' in n:
                p.copy_(src[n])
    assert sum('.final.' in n and n.endswith('.y') for n in src) == L * 2 * (3 if kind == 'esmc' else 2)
    got = three(tokens, pad_args, lora_names=['y'])
    assert torch.equal(got, lone(tokens, pad_args))
    assert not torch.equal(got, three(tokens, pad_args)) and not torch.equal(got, three(tokens, pad_args, lora_names=['x']))
    assert torch.equal(three(tokens, pad_args), three(tokens, pad_args, lora_names=['x', 'y', 'z']))


# ------------------------------------------------------------------ 7. QLoRA

def _twin(tmp_path, kind, q, lora):
    """The bfloat16 model of the same checkpoint that holds the quantised model's expanded weights -- lin.dequantize() in every
    projection and, where the fused forward reads a LayerNorm-folded image (QKV, FFN up), that image with its constants in place of
    the twin's own fold of the expanded weight (the expansion applies the LayerNorm gain before its one rounding to bfloat16; folding
    the rounded weight rounds twice) -- with the same adapters."""
    twin = tiny(tmp_path, kind, L, E, H, SEED)
    with torch.no_grad():
        for (n, a), (m, b) in zip(_projections(twin), _projections(q)):
            assert n == m
            a.weight.data.copy_(b.dequantize())
    twin.invalidate_graphs()
    twin.add_lora(**lora)
    own = dict(twin.named_parameters())
    with torch.no_grad():
        for n, p in q.named_parameters():
            if '.lora_' in n:
                own[n].copy_(p)
    return twin


def _hold_folded_images(twin, q):
    for tl, ql in zip(twin.layers, q.layers):
        for holder, q4 in ((tl.self_attn, ql.self_attn._q4_qkv), (tl, ql._q4_up)):
            holder._pack_fold()
            key = holder._derived.key('fold')
            holder._derived._entries['fold'] = (key, (q4.folded()[0].clone(), q4.c1, q4.c2))


@pytest.mark.parametrize('kind', KINDS)
def test_qlora_all_six_targets(kind, tmp_path):
    lora = dict(rank=8, alpha=16, layers=ALL_SIX)
    path = syn.write_checkpoint(str(tmp_path / f'{kind}_q.safetensors'), f'{kind}_t', L, E, H, seed=SEED)
    torch.manual_seed(1)
    q = ESM.from_pretrained(path, quantization='4bit', device=DEV).add_lora(**lora, quantized_base=True)
    tokens_in, tokens, mask, pad_args = masked_batch(q)
    base = ESM.from_pretrained(path, quantization='4bit', device=DEV)
    assert torch.equal(q(tokens, pad_args), base(tokens, pad_args)), 'fresh adapters over the quantised base change no bit'
    fill_b(q, 1)
    assert not torch.equal(q(tokens, pad_args), base(tokens, pad_args))
    twin = _twin(tmp_path, kind, q, lora)
    # training: the existing criterion, bit-equality with the twin (same GEMM kernel on operands that hold the same bits)
    def step(model):
        model.zero_grad(set_to_none=True)
        logits = model.forward_trainable(tokens_in, pad_args)
        loss = esme.cross_entropy(logits, tokens, mask, alphabet=model.alphabet)
        loss.backward()
        return logits.detach(), loss.detach(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    lq, loss_q, gq = step(q.train())
    lt, loss_t, gt = step(twin.train())
    assert torch.equal(lq, lt) and torch.equal(loss_q, loss_t) and set(gq) == set(gt)
    assert all('.lora_' in n for n in gq) and sum('.final.' in n for n in gq) == L * 2 * (3 if kind == 'esmc' else 2)
    for n in gq:
        assert bool(gq[n].any()) and torch.equal(gq[n], gt[n]), f'gradient of {n} differs from the twin'
    # the fused forward: the unfused form reads the plain expansions, the LayerNorm-folded form the folded images
    q.eval(), twin.eval()
    q.fold_layernorm = twin.fold_layernorm = False
    assert torch.equal(q(tokens, pad_args), twin(tokens, pad_args)), 'unfused form'
    q.fold_layernorm = twin.fold_layernorm = True
    _hold_folded_images(twin, q)
    assert torch.equal(q(tokens, pad_args), twin(tokens, pad_args)), 'LayerNorm-folded form'
    assert torch.equal(q(tokens, pad_args, lora_names=['default']), twin(tokens, pad_args))
    # one optimiser step changes adapter tensors only
    before = {k: v.clone() for k, v in q.state_dict().items()}
    opt = esme.optim.AdamW([p for p in q.parameters() if p.requires_grad], lr=5e-3, weight_decay=0.0)
    step(q.train())
    opt.step()
    changed = [k for k, v in q.state_dict().items() if not torch.equal(v, before[k])]
    assert changed and all('.lora_' in k for k in changed), [k for k in changed if '.lora_' not in k]
    assert any('.final.' in k and '.lora_B.' in k for k in changed)
    out = q.eval()(tokens, pad_args)
    assert bool(torch.isfinite(out.float()).all())
    # nothing of an FFN weight's shape is kept in bfloat16: the adapter cache holds the extension blocks alone
    shapes = {(FF, E), (2 * FF, E), (E, FF)}
    for layer in q.layers:
        held = [t for holder in (layer, layer.final[1] if kind == 'esmc' else layer) for t in holder._derived.tensors()]
        for _, m in (*layer._ffn_projections()[0], layer._ffn_projections()[1]):
            held += list(m._derived.tensors()) + (list(m.layer._derived.tensors()) if getattr(m.layer, '_derived', None) is not None else [])
        assert held, 'the extension blocks are cached'
        for t in held:
            assert not (t.dtype == torch.bfloat16 and t.dim() == 2 and any(t.shape[0] == r and t.shape[1] >= c for r, c in shapes)), tuple(t.shape)
    Xu, Xd = q.layers[0].ffn_lora_ext_widths(None)
    Xq, Xo = q.layers[0].self_attn.lora_ext_widths(None)
    layer = q.layers[0]
    packed = [layer._q4_up.rows * (layer._q4_up.cols + Xu), layer._q4_down.rows * (layer._q4_down.cols + Xd),
              layer.self_attn._q4_qkv.rows * (layer.self_attn._q4_qkv.cols + Xq), layer.self_attn._q4_out.rows * (layer.self_attn._q4_out.cols + Xo)]
    assert q._q4_scratch.buf.numel() == max(packed), 'the weight scratch is the largest expanded matrix with its extension columns'
