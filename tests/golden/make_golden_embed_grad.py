#!/usr/bin/env python
"""Golden fixture for masked-LM training: the gradient of the token-embedding table of one masked-token
training step, from this project's oracle alone (runs on the CPU in a few seconds).

    python tests/golden/make_golden_embed_grad.py     # rewrites g17_embed_grad.npz

make_golden_full_grad.py's recipe with `embed_tokens.weight` as an extra leaf: the two models of tests/test_lora_gpu.golden_model
without adapters on the batch of g14_lora_grad.npz, every projection, LayerNorm and the table trained.

 - `{kind}_oracle/loss`, `{kind}_oracle/embed_tokens.weight`: float64 autograd of torch's cross entropy through oracle/esm_oracle.py
   with the parameters' bfloat16 values as float64 leaves -- the truth, stored as float64 (33 / 64 rows: small).
 - `{kind}_bf16_error/embed_tokens.weight`: the relative (Frobenius) error against that truth of the SAME data flow in bfloat16 torch
   ops (golden_util.exact_cpu_gemms; the table's gradient is torch's own bfloat16 index backward).  A test's bar is twice this.
 - `{kind}_rows`: how many rows of the batch hold each id (the fan-in of each table row).
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
import make_golden_full_grad as FG                       # noqa: E402

KINDS = ('esm2', 'esmc')
NAME = 'embed_tokens.weight'


def step(weights, heads, dtype, tokens_in, tokens, mask, cu, ml):
    """(loss, gradients) with the table as a leaf next to make_golden_full_grad's."""
    leaves = {k: v.to(dtype).clone().requires_grad_() for k, v in weights.items() if FG.is_trained(k) or k == NAME}
    w = {k: leaves[k] if k in leaves else v.to(dtype) for k, v in weights.items()}
    with exact_cpu_gemms(dtype == torch.bfloat16):
        logits = O.forward_logits(w, heads, tokens_in, cu, ml, dtype=dtype)
        loss = torch.nn.functional.cross_entropy(logits[mask], tokens[mask], ignore_index=O.PAD_IDX)
        loss.backward()
    return loss.detach(), {k: p.grad for k, p in leaves.items()}


def main():
    g13, g14 = load_golden('g13_lora.npz'), load_golden('g14_lora_grad.npz')
    cu, ml = g14['cu_lens'], int(g14['max_len'])
    out = {}
    for kind in KINDS:
        L, E, H, seed = (int(g13[f'{kind}_{k}']) for k in ('L', 'E', 'H', 'seed'))
        weights = syn.synthetic_state_dict(kind, L, E, seed)
        args = (g14[f'{kind}_tokens_in'], g14[f'{kind}_tokens'], g14[f'{kind}_mask'], cu, ml)
        loss64, g64 = step(weights, H, torch.float64, *args)
        loss16, g16 = step(weights, H, torch.bfloat16, *args)
        bar = FG.rel(g16[NAME], g64[NAME])
        out[f'{kind}_oracle/loss'] = np.float64(loss64)
        out[f'{kind}_oracle/{NAME}'] = g64[NAME].numpy()
        out[f'{kind}_bf16_error/{NAME}'] = np.float64(bar)
        out[f'{kind}_rows'] = torch.bincount(g14[f'{kind}_tokens_in'], minlength=weights[NAME].shape[0]).numpy().astype(np.int32)
        print(f'  {kind}: table {tuple(g64[NAME].shape)}, largest fan-in {int(out[f"{kind}_rows"].max())}; loss f64 {float(loss64):.8f}, '
              f'bf16 {float(loss16):.5f}; bf16 against f64: {bar:.4f}')
    path = os.path.join(HERE, 'g17_embed_grad.npz')
    np.savez_compressed(path, **out)
    print(f'  g17_embed_grad.npz {os.path.getsize(path) / 1024:8.1f} KiB')
    assert os.path.getsize(path) < 1_000_000


if __name__ == '__main__':
    main()
