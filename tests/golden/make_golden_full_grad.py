#!/usr/bin/env python
"""Golden fixture for full fine-tuning: the loss and the gradient of every projection weight, bias and
LayerNorm parameter of one masked-token training step, from this project's oracle alone (runs on the CPU in a few seconds).

    python tests/golden/make_golden_full_grad.py     # rewrites g15_full_grad.npz and g15_full_grad_esmc.npz

For the two models of tests/test_lora_gpu.golden_model WITHOUT adapters (the synthetic checkpoints of g13's L, E, H and seed) on the
batch of g14_lora_grad.npz (tokens, the masked input, the mask, cu_lens):

 - `{kind}_oracle/loss`, `{kind}_oracle/{name}`: float64 autograd of torch's cross entropy through oracle/esm_oracle.py with the
   parameters' bfloat16 values as float64 leaves -- the truth.  A tensor is stored as float16 after scaling by a power of two that
   brings its largest magnitude into [1, 2) (`{kind}_oracle_exp/{name}` holds the exponent): 2^-11 relative per element, about 2e-4 in
   relative Frobenius error, two orders below the bars, which a float32 copy of the 0.9 M gradient elements would not fit next to
   (no committed file may exceed 1 MiB; for the same reason the ESM-C tensors live in a file of their own).
 - `{kind}_bf16_error/loss`, `{kind}_bf16_error/{name}`: the relative (Frobenius) error against that truth of the SAME data flow in
   bfloat16 torch ops -- the oracle run with dtype=bfloat16 and bfloat16 leaves under golden_util.exact_cpu_gemms (every GEMM summed
   in float64 and rounded once, so the numbers do not depend on the processor).  A test's bar is twice this: two independent bf16
   pipelines against one truth err by that size each.
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
from golden_util import exact_cpu_gemms, load_golden     # noqa: E402

KINDS = ('esm2', 'esmc')


def is_trained(k):
    """A layer's projections and LayerNorms, and emb_layer_norm_after: what model.mark_trainable() selects."""
    return k.startswith('layers.') or k.startswith('emb_layer_norm_after.')


def step(weights, heads, dtype, tokens_in, tokens, mask, cu, ml):
    leaves = {k: v.to(dtype).clone().requires_grad_() for k, v in weights.items() if is_trained(k)}
    w = {k: leaves[k] if k in leaves else v.to(dtype) for k, v in weights.items()}
    with exact_cpu_gemms(dtype == torch.bfloat16):
        logits = O.forward_logits(w, heads, tokens_in, cu, ml, dtype=dtype)
        loss = torch.nn.functional.cross_entropy(logits[mask], tokens[mask], ignore_index=O.PAD_IDX)
        loss.backward()
    return loss.detach(), {k: p.grad for k, p in leaves.items()}


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def pack16(t):
    """(float16 mantissas, exponent e): t = mantissas * 2^e, the largest magnitude in [1, 2)."""
    m = float(t.abs().max())
    e = int(np.floor(np.log2(m))) if m > 0 else 0
    return (t * 2.0 ** -e).to(torch.float16).numpy(), np.int32(e)


def main():
    g13, g14 = load_golden('g13_lora.npz'), load_golden('g14_lora_grad.npz')
    cu, ml = g14['cu_lens'], int(g14['max_len'])
    files = {'esm2': {'cu_lens': cu.numpy(), 'max_len': ml}, 'esmc': {}}
    for kind in KINDS:
        L, E, H, seed = (int(g13[f'{kind}_{k}']) for k in ('L', 'E', 'H', 'seed'))
        weights = syn.synthetic_state_dict(kind, L, E, seed)
        assert all(v.dtype == torch.bfloat16 for v in weights.values())
        args = (g14[f'{kind}_tokens_in'], g14[f'{kind}_tokens'], g14[f'{kind}_mask'], cu, ml)
        loss64, g64 = step(weights, H, torch.float64, *args)
        loss16, g16 = step(weights, H, torch.bfloat16, *args)
        assert set(g64) == set(g16) and all(v is not None for v in g64.values())
        bars = {k: rel(g16[k], g64[k]) for k in g64}
        main_file, out = files['esm2'], files[kind]
        for k in ('tokens', 'tokens_in', 'mask'):
            main_file[f'{kind}_{k}'] = g14[f'{kind}_{k}'].numpy()
        main_file[f'{kind}_oracle/loss'] = np.float64(loss64)
        main_file[f'{kind}_bf16_error/loss'] = np.float64(abs(float(loss16) - float(loss64)) / abs(float(loss64)))
        worst_store = 0.0
        for k in sorted(g64):
            out[f'{kind}_oracle/{k}'], e = pack16(g64[k])
            main_file[f'{kind}_oracle_exp/{k}'] = e
            main_file[f'{kind}_bf16_error/{k}'] = np.float64(bars[k])
            worst_store = max(worst_store, rel(torch.from_numpy(out[f'{kind}_oracle/{k}']).double() * 2.0 ** int(e), g64[k]))
        print(f'  {kind}: {len(g64)} tensors, {sum(v.numel() for v in g64.values())} elements; loss f64 {float(loss64):.8f}, bf16 {float(loss16):.5f}; '
              f'bf16 against f64: {min(bars.values()):.4f} .. {max(bars.values()):.4f}; float16 storage: worst {worst_store:.1e}')
        assert worst_store < 5e-4 and worst_store < 0.05 * min(bars.values())
    for name, data in (('g15_full_grad.npz', files['esm2']), ('g15_full_grad_esmc.npz', files['esmc'])):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **data)
        size = os.path.getsize(path)
        print(f'  {name} {size / 1024:8.1f} KiB')
        assert size < 1_000_000, name


if __name__ == '__main__':
    main()
