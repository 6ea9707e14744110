#!/usr/bin/env python
"""Golden fixture for LoRA fine-tuning: losses and gradients of one masked-token training step, generated in the
authoring container from the REFERENCE (needs the reference checkout make_golden.py imports; never runs on the GPU box) and from this
project's oracle.  Same rules as make_golden.py: only inputs and recorded results are stored, nothing of the reference's source.

    python tests/golden/make_golden_lora_grad.py     # rewrites g14_lora_grad.npz

For the two models of make_golden_lora.CONFIGS with the g13 adapters (the same seeded fill), a seeded 30 % mask (the masked
positions of the input carry `<mask>`, the targets are the original tokens) and the reference's own `cross_entropy`:

 - `{kind}_ref_f32/...`, `{kind}_ref_bf16/...`: the loss and the gradient of every adapter tensor from the reference's model, loss
   and torch.autograd, in fp32 and in its default bf16 (under exact_cpu_gemms, like every bf16 fixture), the LM head trainable too;
   of the head's own tensors only `{kind}_ref_bf16_error/...`, the relative Frobenius error of the reference's bf16 gradient against
   its fp32 gradient, is kept (the file stays under 1 MB; their fp32 gradients are asserted against the oracle here, at 1e-5);
 - `{kind}_oracle/...`: the same from float64 autograd through oracle/esm_oracle.py on merged weights W + s B A with A and B (and the
   head's tensors) as leaves (stored as float32: 6e-8 relative, two orders below anything a test compares them at).

THE ROTARY SEAM.  The reference's rotary autograd wrapper (its esme/rotary.py, ApplyRotaryEmbQKV_.backward) applies the FORWARD
rotation to the incoming gradients instead of the inverse rotation, so its q / k gradients -- and every adapter gradient behind a
rotary -- are wrong by the order of the gradient itself (the loss is right).  The reference numbers stored here
are taken with `apply_rotary_emb_qkv_` replaced at run time by the reference's own plain `apply_rotary` (the same forward, torch takes
the backward); the script asserts both statements: with the seam as shipped the worst adapter gradient is off by more than 10 %, with
the replacement every tensor agrees with the oracle to 1e-5.  The truth for gradients in this project is the oracle's float64 autograd.
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg          # noqa: E402  (flash_attn stand-in, synthetic weights, helpers)
import make_golden_lora as mgl    # noqa: E402  (CONFIGS, NAMES, LENGTHS, fill_adapters)

sys.path.insert(0, mg.ROOT)
from oracle import esm_oracle as O      # noqa: E402

MASK_FRACTION = 0.3


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def is_trained(k):
    return '.lora_A.' in k or '.lora_B.' in k or k.startswith('lm_head.')


def masked_batch(tokens, seed, mask_idx):
    """(input with `<mask>` at the masked positions, boolean mask): numpy PCG64, exactly round(0.3 T) positions."""
    rng = np.random.Generator(np.random.PCG64(seed))
    T = tokens.numel()
    pos = np.sort(rng.permutation(T)[:int(round(MASK_FRACTION * T))])
    mask = torch.zeros(T, dtype=torch.bool)
    mask[torch.from_numpy(pos)] = True
    return torch.where(mask, torch.full_like(tokens, mask_idx), tokens), mask


def reference_step(ref, syn, kind, c, dt, tokens_in, tokens, mask, cu, ml):
    """(loss, {name: grad}) of the reference model with the g13 adapters and a trainable LM head."""
    from esme.alphabet import Alphabet, Alphabet3
    from esme.loss import cross_entropy
    model = mg.build_ref_model(ref, syn, kind, c['L'], c['E'], c['H'], c['seed'], dt)
    model.add_lora(rank=c['rank'], alpha=c['alpha'], layers=c['layers'], adapter_names=list(mgl.NAMES))
    mgl.fill_adapters(model, c['seed'] + 1000, c['b_scale'])
    model.mark_lmhead(True)
    model.train()
    with mg.exact_cpu_gemms(dt == torch.bfloat16):
        loss = cross_entropy(model(tokens_in, (cu, ml)), tokens, mask, alphabet=Alphabet if kind == 'esm2' else Alphabet3)
        loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.requires_grad}
    assert grads and all(is_trained(k) for k in grads), sorted(k for k in grads if not is_trained(k))
    return loss.detach(), grads, {k: p.detach().clone() for k, p in model.named_parameters()}


def oracle_step(kind, c, params, tokens_in, tokens, mask, cu, ml):
    """float64 autograd through oracle/esm_oracle.py: merged weights W + s B A, the adapters and the head's tensors as leaves."""
    s = c['alpha'] / c['rank']
    leaves = {k: v.double().clone().requires_grad_() for k, v in params.items() if is_trained(k)}
    weights = {}
    for k, v in params.items():
        if is_trained(k) and not k.startswith('lm_head.'):
            continue
        if k.endswith('.layer.weight'):                              # a wrapped projection: merge its adapters
            base = k[:-len('.layer.weight')]
            w = v.double()
            for n in mgl.NAMES:
                w = w + s * (leaves[f'{base}.lora_B.{n}'] @ leaves[f'{base}.lora_A.{n}'])
            weights[base + '.weight'] = w
        elif k.endswith('.layer.bias'):
            weights[k[:-len('.layer.bias')] + '.bias'] = v.double()
        else:
            weights[k] = leaves[k] if k in leaves else v.double()
    logits = O.forward_logits(weights, c['H'], tokens_in, cu, ml, dtype=torch.float64)
    loss = torch.nn.functional.cross_entropy(logits[mask], tokens[mask], ignore_index=O.PAD_IDX)
    loss.backward()
    return loss.detach(), {k: p.grad for k, p in leaves.items()}


def main():
    ref = mg.import_reference()
    syn = mg.load_synthetic()
    import esme.rotary as ref_rotary
    import esme.esm as ref_esm
    ref_esm.tqdm = lambda it, *a, **k: it
    shipped = ref_rotary.apply_rotary_emb_qkv_

    def plain(q, k, cos, sin, cu_lens):                              # the reference's own apply_rotary; torch differentiates it
        return ref_rotary.apply_rotary(q, cos, sin, cu_lens), ref_rotary.apply_rotary(k, cos, sin, cu_lens)

    cu, ml = syn.cu_lens_of(mgl.LENGTHS), max(mgl.LENGTHS)
    g = {'lengths': np.asarray(mgl.LENGTHS), 'cu_lens': cu.numpy(), 'max_len': ml, 'mask_fraction': MASK_FRACTION}
    for kind, c in mgl.CONFIGS.items():
        tokens = syn.random_tokens(mgl.LENGTHS, seed=c['seed'])
        tokens_in, mask = masked_batch(tokens, c['seed'] + 2000, O.MASK_IDX)
        g[f'{kind}_tokens'], g[f'{kind}_tokens_in'], g[f'{kind}_mask'] = tokens.numpy(), tokens_in.numpy(), mask.numpy()
        args = (tokens_in, tokens, mask, cu, ml)
        ref_rotary.apply_rotary_emb_qkv_ = plain
        try:
            loss32, g32, params = reference_step(ref, syn, kind, c, torch.float32, *args)
            loss16, g16, _ = reference_step(ref, syn, kind, c, torch.bfloat16, *args)
        finally:
            ref_rotary.apply_rotary_emb_qkv_ = shipped
        _, g32_shipped, _ = reference_step(ref, syn, kind, c, torch.float32, *args)
        loss64, g64 = oracle_step(kind, c, params, *args)
        assert set(g32) == set(g16) == set(g64)
        worst = max(rel(g32[k], g64[k]) for k in g64)
        worst_shipped = max(rel(g32_shipped[k], g64[k]) for k in g64)
        bar = {k: rel(g16[k].float(), g32[k]) for k in g64}
        print(f'  {kind}: loss f64 {float(loss64):.8f}, fp32 - f64 {float(loss32) - float(loss64):.1e}, bf16 {float(loss16):.5f}; fp32 gradients against '
              f'the oracle: worst {worst:.1e} (rotary seam as shipped: {worst_shipped:.2f}); bf16 against fp32: {min(bar.values()):.4f} .. {max(bar.values()):.4f}')
        assert abs(float(loss32) - float(loss64)) < 1e-6 and worst < 1e-5, (kind, worst)
        assert worst_shipped > 0.1, 'the reference\'s rotary backward agrees with autograd: the seam note in DESIGN.md is out of date'
        g[f'{kind}_ref_f32/loss'], g[f'{kind}_ref_bf16/loss'], g[f'{kind}_oracle/loss'] = np.float32(loss32), np.float32(loss16.float()), np.float64(loss64)
        for k in sorted(g64):
            g[f'{kind}_oracle/{k}'] = g64[k].float().numpy()
            if k.startswith('lm_head.'):                             # (the file's size: the head's reference gradients enter as their error only)
                g[f'{kind}_ref_bf16_error/{k}'] = np.float64(bar[k])
            else:
                g[f'{kind}_ref_f32/{k}'] = g32[k].numpy()
                g[f'{kind}_ref_bf16/{k}'] = mg.bits(g16[k])
    path = os.path.join(HERE, 'g14_lora_grad.npz')
    np.savez_compressed(path, **g)
    size = os.path.getsize(path)
    print(f'  g14_lora_grad.npz {size / 1024:8.1f} KiB')
    assert size < 1_000_000


if __name__ == '__main__':
    main()
