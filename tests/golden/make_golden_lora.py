#!/usr/bin/env python
"""Golden fixtures for the LoRA adapters, generated from the REFERENCE imported in the authoring
container (needs the reference checkout make_golden.py imports; never runs on the GPU box).  Same rules as make_golden.py: only inputs and the reference's own
outputs are stored, nothing of its source.

    python tests/golden/make_golden_lora.py     # rewrites g13_lora_esm2.safetensors, g13_lora_esmc.safetensors, g13_lora.npz

 - g13_lora_{esm2,esmc}.safetensors: the files the reference's own `save_lora` wrote for reference models built from
   esme.synthetic checkpoints, after its own `add_lora` and a seeded fill of lora_A / lora_B (tiny ESM-2: adapters 'a', 'b' of rank 16,
   alpha 16 on query / value / output; tiny ESM-C: rank 8, alpha 12 -- alpha / rank = 1.5, not a power of two -- on all four);
 - g13_lora.npz: tokens, cu_lens, the 2-D padded tokens, and per model the reference's logits in fp32 and bf16 for lora_names = None,
   ['a'], ['b'], ['a', 'b'], the 2-D logits for None, the logits WITHOUT adapters, and layer-0 q / k / v / attention-branch taps.

The scale of lora_B is chosen so that every adapter selection moves the fp32 logits by at least 10 x the parity floor of
tests/test_model_gpu.py::assert_parity (4e-3 relative Frobenius), and different selections differ by as much: a forward that drops,
swaps or mis-selects an adapter cannot pass.  The script asserts it.
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg          # noqa: E402  (flash_attn stand-in, synthetic weights, helpers)

CONFIGS = {
    'esm2': dict(L=2, E=128, H=4, seed=31, rank=16, alpha=16, layers=('query', 'value', 'output'), b_scale=0.25),
    'esmc': dict(L=2, E=128, H=2, seed=32, rank=8, alpha=12, layers=('query', 'key', 'value', 'output'), b_scale=0.25),
}
NAMES = ['a', 'b']
CASES = {'none': None, 'a': ['a'], 'b': ['b'], 'ab': ['a', 'b']}
LENGTHS = [9, 40, 23]
FLOOR = 4e-3


def fill_adapters(model, seed, b_scale):
    """lora_A ~ N(0, 1) / sqrt(in), lora_B ~ N(0, 1) * b_scale / sqrt(rank), rounded to bf16, from numpy PCG64 in state-dict order."""
    rng = np.random.Generator(np.random.PCG64(seed))
    for k, p in sorted(model.named_parameters()):
        if '.lora_A.' in k:
            v = rng.standard_normal(tuple(p.shape), dtype=np.float32) / np.sqrt(p.shape[1])
        elif '.lora_B.' in k:
            v = rng.standard_normal(tuple(p.shape), dtype=np.float32) * b_scale / np.sqrt(p.shape[1])
        else:
            continue
        p.data.copy_(torch.from_numpy(v).bfloat16().to(p.dtype))


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def main():
    torch.set_grad_enabled(False)
    ref = mg.import_reference()
    syn = mg.load_synthetic()
    import esme.esm as ref_esm
    ref_esm.tqdm = lambda it, *a, **k: it
    g = {'lengths': np.asarray(LENGTHS)}          # (adapter names and tapped projections are in the safetensors metadata)
    cu = syn.cu_lens_of(LENGTHS)
    ml = max(LENGTHS)
    g.update(cu_lens=cu.numpy(), max_len=ml)
    for kind, c in CONFIGS.items():
        tokens = syn.random_tokens(LENGTHS, seed=c['seed'])
        pad_idx = 1
        tok2d = torch.full((len(LENGTHS), ml), pad_idx, dtype=torch.int64)
        for i, (a, b) in enumerate(zip(cu[:-1].tolist(), cu[1:].tolist())):
            tok2d[i, :b - a] = tokens[a:b]
        g[f'{kind}_tokens'], g[f'{kind}_tokens2d'] = tokens.numpy(), tok2d.numpy()
        for key in ('L', 'E', 'H', 'seed', 'rank', 'alpha'):
            g[f'{kind}_{key}'] = c[key]
        logits32 = {}
        for dt, tag in ((torch.float32, 'f32'), (torch.bfloat16, 'bf16')):
            model = mg.build_ref_model(ref, syn, kind, c['L'], c['E'], c['H'], c['seed'], dt)
            with mg.exact_cpu_gemms(dt == torch.bfloat16):
                base = model(tokens, (cu, ml))
            g[f'{kind}_logits_base_{tag}'] = mg.f32(base)
            model.add_lora(rank=c['rank'], alpha=c['alpha'], layers=c['layers'], adapter_names=list(NAMES))
            model.eval()
            with mg.exact_cpu_gemms(dt == torch.bfloat16):
                fresh = model(tokens, (cu, ml))
            assert torch.equal(fresh, base), 'fresh adapters (lora_B = 0) must not move the reference'
            fill_adapters(model, c['seed'] + 1000, c['b_scale'])
            if dt == torch.bfloat16:
                model.save_lora(os.path.join(HERE, f'g13_lora_{kind}.safetensors'))
            with mg.exact_cpu_gemms(dt == torch.bfloat16):
                for case, names in CASES.items():
                    y = model(tokens, (cu, ml), lora_names=names)
                    g[f'{kind}_logits_{case}_{tag}'] = mg.f32(y)
                    if dt == torch.float32:
                        logits32[case] = y
                g[f'{kind}_logits2d_none_{tag}'] = mg.f32(model(tok2d))
                # layer-0 taps with all adapters: q / k / v as the reference's _qkv returns them (before rotary; ESM-C: after its q / k
                # LayerNorm), and the attention branch's output (out-projection with its adapters, before the residual add)
                x0 = model.embedding(tokens, (cu, ml))
                att = model.layers[0].self_attn
                q, k, v = att._qkv(x0, NAMES)
                T = x0.shape[0]
                for nm, t in (('q', q), ('k', k), ('v', v)):
                    g[f'{kind}_tap_{nm}_{tag}'] = mg.f32(t.reshape(T, -1).contiguous())
                g[f'{kind}_tap_attn_out_{tag}'] = mg.f32(att(x0, cu, ml, NAMES))
            if dt == torch.float32:
                assert torch.equal(logits32['none'], logits32['ab']), 'None applies all adapters'
                moved = {case: rel(logits32[case], base) for case in ('a', 'b', 'ab')}
                apart = {'a-b': rel(logits32['a'], logits32['b']), 'a-ab': rel(logits32['a'], logits32['ab']),
                         'b-ab': rel(logits32['b'], logits32['ab'])}
                print(f'  {kind}: adapters move the fp32 logits by {moved}, selections differ by {apart} (floor {FLOOR})')
                assert min(*moved.values(), *apart.values()) >= 10 * FLOOR, (kind, moved, apart)
    np.savez_compressed(os.path.join(HERE, 'g13_lora.npz'), **g)
    for fn in ('g13_lora_esm2.safetensors', 'g13_lora_esmc.safetensors', 'g13_lora.npz'):
        size = os.path.getsize(os.path.join(HERE, fn))
        print(f'  {fn:28s} {size / 1024:8.1f} KiB')
        assert size < 1_000_000, fn


if __name__ == '__main__':
    main()
