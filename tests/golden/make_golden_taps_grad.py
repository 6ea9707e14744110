#!/usr/bin/env python
"""Golden fixture for training through layer taps: the tapped representation and the gradients of a
loss over all of its columns, from this project's oracle alone (runs on the CPU in under a minute).

    python tests/golden/make_golden_taps_grad.py     # rewrites g17_taps_grad.npz and g17_taps_grad_esmc.npz

Two synthetic models of 3 layers, E = 128, 2 heads (ESM-2 and ESM-C: head dim 64) on six packed sequences of 1, 2, 63, 64, 65 and
129 tokens.  The representation is oracle/esm_oracle.forward_representation(layers=[0, 2]): the final-LayerNorm output followed by
the raw outputs of layers 0 and 2, (T, 3 E).  The loss is sum(w * rep) with w = `loss_weights(T, 3 E)` (numpy PCG64, float32: the
tests draw the same numbers from the same seed, so w is not stored).

 - `{kind}_taps`, `{kind}_taps_exp`: the two tap blocks (T, 2 E) of the model without adapters in float64, stored like g15's tensors
   (float16 after scaling by a power of two, the exponent beside them); `{kind}_taps_bf16_error`: per block, the relative (Frobenius)
   error of the same data flow in bfloat16 torch ops (the oracle with dtype=bfloat16 under golden_util.exact_cpu_gemms).
 - case `lora`: adapters of rank 4 (alpha 8) on query / value / output of every layer, filled from numpy PCG64 as
   make_golden_lora.fill_adapters does and stored as bfloat16 bits under `{kind}_lora/{name}`; `{kind}_lora_oracle/{name}`: float64
   autograd through the oracle on merged weights W + s B A with A and B as leaves (stored as float32);
   `{kind}_lora_bf16_error/{name}`: the error of the bfloat16 flow against it, the merged weight rounded to bfloat16.
 - case `top`: the projections and LayerNorms of the last layer as leaves (what mark_trainable(layers=[-1]) selects):
   `{kind}_top_oracle/{name}` + `{kind}_top_oracle_exp/{name}` (float16 + exponent, as g15), `{kind}_top_bf16_error/{name}`.
A test's bar is twice the bf16 error, g15's construction: two independent bf16 pipelines against one truth err by that size each.
The ESM-C tensors live in a file of their own (no committed file may exceed 1 MiB).
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'esm-efficient_amd'), os.path.dirname(HERE)):
    sys.path.insert(0, p)
from oracle import esm_oracle as O                       # noqa: E402
from esme import synthetic as syn                        # noqa: E402
from golden_util import exact_cpu_gemms                  # noqa: E402
from make_golden_full_grad import pack16, rel            # noqa: E402

KINDS = ('esm2', 'esmc')
L, E, H = 3, 128, 2
SEEDS = {'esm2': 41, 'esmc': 42}
LENGTHS = (1, 2, 63, 64, 65, 129)
LAYERS = (0, 2)
RANK, ALPHA, B_SCALE = 4, 8, 0.25
PROJ = ('q', 'v', 'out')                                 # add_lora(layers=('query', 'value', 'output'))
ADAPTER = 'default'
W_SEED = 1700


def loss_weights(T, C):
    """w (T, C) float32, the same on every machine (numpy PCG64)."""
    return torch.from_numpy(np.random.Generator(np.random.PCG64(W_SEED)).standard_normal((T, C), dtype=np.float32))


def adapters(seed):
    """{state-dict key: bfloat16 tensor}: lora_A ~ N(0, 1) / sqrt(in), lora_B ~ N(0, 1) * B_SCALE / sqrt(rank), in sorted key order."""
    rng = np.random.Generator(np.random.PCG64(seed))
    keys = sorted(f'layers.{i}.self_attn.{p}.lora_{ab}.{ADAPTER}' for i in range(L) for p in PROJ for ab in 'AB')
    out = {}
    for k in keys:
        if '.lora_A.' in k:
            v = rng.standard_normal((RANK, E), dtype=np.float32) / np.sqrt(E)
        else:
            v = rng.standard_normal((E, RANK), dtype=np.float32) * B_SCALE / np.sqrt(RANK)
        out[k] = torch.from_numpy(v).bfloat16()
    return out


def merged(weights, leaves, dtype):
    """The model's weights with W + s B A in place of every adapted projection, in `dtype` (bfloat16: the sum is formed in float32
    and rounded once)."""
    w = {k: v.to(dtype) for k, v in weights.items()}
    s = ALPHA / RANK
    for i in range(L):
        for p in PROJ:
            base = f'layers.{i}.self_attn.{p}'
            a, b = leaves[f'{base}.lora_A.{ADAPTER}'], leaves[f'{base}.lora_B.{ADAPTER}']
            wide = torch.float64 if dtype == torch.float64 else torch.float32
            w[base + '.weight'] = (weights[base + '.weight'].to(wide) + s * (b.to(wide) @ a.to(wide))).to(dtype)
    return w


def run(w, tokens, cu, ml, dtype, wts):
    with exact_cpu_gemms(dtype == torch.bfloat16):
        rep = O.forward_representation(w, H, tokens, cu, ml, dtype=dtype, layers=LAYERS)
        loss = (rep.double() * wts.double()).sum()
    return rep, loss


def lora_step(weights, ad, tokens, cu, ml, dtype, wts):
    leaves = {k: v.to(dtype).clone().requires_grad_() for k, v in ad.items()}
    _, loss = run(merged(weights, leaves, dtype), tokens, cu, ml, dtype, wts)
    loss.backward()
    return {k: p.grad for k, p in leaves.items()}


def top_step(weights, tokens, cu, ml, dtype, wts):
    leaves = {k: v.to(dtype).clone().requires_grad_() for k, v in weights.items() if k.startswith(f'layers.{L - 1}.')}
    rep, loss = run({k: leaves[k] if k in leaves else v.to(dtype) for k, v in weights.items()}, tokens, cu, ml, dtype, wts)
    loss.backward()
    return rep.detach(), {k: p.grad for k, p in leaves.items()}


def main():
    cu, ml = syn.cu_lens_of(list(LENGTHS)), max(LENGTHS)
    T = int(cu[-1])
    wts = loss_weights(T, (1 + len(LAYERS)) * E)
    files = {'esm2': {'lengths': np.asarray(LENGTHS), 'cu_lens': cu.numpy(), 'max_len': ml, 'layers': np.asarray(LAYERS), 'L': L, 'E': E, 'H': H,
                      'rank': RANK, 'alpha': ALPHA, 'w_seed': W_SEED}, 'esmc': {}}
    for kind in KINDS:
        seed = SEEDS[kind]
        main_file, out = files['esm2'], files[kind]
        weights = syn.synthetic_state_dict(kind, L, E, seed)
        tokens = syn.random_tokens(list(LENGTHS), seed=seed)
        main_file[f'{kind}_seed'], main_file[f'{kind}_tokens'] = seed, tokens.numpy()
        args = (tokens, cu, ml)
        rep64, g64 = top_step(weights, *args, torch.float64, wts)
        rep16, g16 = top_step(weights, *args, torch.bfloat16, wts)
        out[f'{kind}_taps'], main_file[f'{kind}_taps_exp'] = pack16(rep64[:, E:])
        main_file[f'{kind}_taps_bf16_error'] = np.asarray([rel(rep16[:, (1 + j) * E:(2 + j) * E], rep64[:, (1 + j) * E:(2 + j) * E]) for j in range(len(LAYERS))])
        bars = {k: rel(g16[k], g64[k]) for k in g64}
        worst_store = 0.0
        for k in sorted(g64):
            out[f'{kind}_top_oracle/{k}'], e = pack16(g64[k])
            main_file[f'{kind}_top_oracle_exp/{k}'] = e
            main_file[f'{kind}_top_bf16_error/{k}'] = np.float64(bars[k])
            worst_store = max(worst_store, rel(torch.from_numpy(out[f'{kind}_top_oracle/{k}']).double() * 2.0 ** int(e), g64[k]))
        assert worst_store < 5e-4 and worst_store < 0.05 * 2 * min(bars.values()), (worst_store, min(bars.values()))      # under 5 % of the smallest bar
        print(f'  {kind} top: {len(g64)} tensors, {sum(v.numel() for v in g64.values())} elements; bf16 against f64: {min(bars.values()):.4f} .. '
              f'{max(bars.values()):.4f}; taps bf16 against f64: {main_file[f"{kind}_taps_bf16_error"]}; float16 storage: worst {worst_store:.1e}')
        ad = adapters(seed + 1000)
        a64 = lora_step(weights, ad, *args, torch.float64, wts)
        a16 = lora_step(weights, ad, *args, torch.bfloat16, wts)
        bars = {k: rel(a16[k], a64[k]) for k in a64}
        for k in sorted(a64):
            out[f'{kind}_lora/{k}'] = ad[k].view(torch.int16).numpy().view(np.uint16)
            out[f'{kind}_lora_oracle/{k}'] = a64[k].float().numpy()
            main_file[f'{kind}_lora_bf16_error/{k}'] = np.float64(bars[k])
        print(f'  {kind} lora: {len(a64)} tensors; bf16 against f64: {min(bars.values()):.4f} .. {max(bars.values()):.4f}')
    for name, data in (('g17_taps_grad.npz', files['esm2']), ('g17_taps_grad_esmc.npz', files['esmc'])):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **data)
        size = os.path.getsize(path)
        print(f'  {name} {size / 1024:8.1f} KiB')
        assert size < 1_000_000, name


if __name__ == '__main__':
    main()
