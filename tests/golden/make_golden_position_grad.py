#!/usr/bin/env python
"""Golden fixture for training the learned-position models: the gradients of the position table, the
token table, ESM-1b's emb_layer_norm_before and one projection of one masked-token training step, from this project's oracle alone
(runs on the CPU in a few seconds).

    python tests/golden/make_golden_position_grad.py     # rewrites g18_position_grad.npz

make_golden_embed_grad.py's recipe on tiny ESM-1b and ESM-1v models (g13's ESM-2 depth, width and seed, H = 2: the head dim 64 of
the released models) and its batch (g14_lora_grad.npz's ESM-2 batch: the alphabet is the same), with `embed_positions.weight`,
`embed_tokens.weight` and `emb_layer_norm_before.*` as extra leaves next to make_golden_full_grad's.

 - `{kind}_oracle/loss`, `{kind}_oracle/{name}`: float64 autograd of torch's cross entropy through oracle/esm_oracle.py with the
   parameters' bfloat16 values as float64 leaves -- the truth, stored as float64.  Of the (4098, E) position table only the first
   max_len + 2 rows are stored: the oracle's gradient of every other row is exactly zero (asserted here).
 - `{kind}_bf16_error/{name}`: the relative (Frobenius) error against that truth of the SAME data flow in bfloat16 torch ops
   (golden_util.exact_cpu_gemms; the tables' gradients are torch's own bfloat16 index backward).  A test's bar is twice this.
 - `{kind}_fan_in`: how many sequences of the batch reach each stored row of the position table.
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

KINDS = ('esm1b', 'esm1v')
HEADS = 2
POS, TOK, PROJ = 'embed_positions.weight', 'embed_tokens.weight', 'layers.0.self_attn.q.weight'
NORM = ('emb_layer_norm_before.weight', 'emb_layer_norm_before.bias')


def stored(kind):
    return (POS, TOK, PROJ) + (NORM if kind == 'esm1b' else ())


def step(weights, heads, dtype, tokens_in, tokens, mask, cu, ml):
    """(loss, gradients) with the two tables and the first LayerNorm as leaves next to make_golden_full_grad's."""
    leaves = {k: v.to(dtype).clone().requires_grad_() for k, v in weights.items() if FG.is_trained(k) or k in (POS, TOK) + NORM}
    w = {k: leaves[k] if k in leaves else v.to(dtype) for k, v in weights.items()}
    with exact_cpu_gemms(dtype == torch.bfloat16):
        logits = O.forward_logits(w, heads, tokens_in, cu, ml, dtype=dtype)
        loss = torch.nn.functional.cross_entropy(logits[mask], tokens[mask], ignore_index=O.PAD_IDX)
        loss.backward()
    return loss.detach(), {k: p.grad for k, p in leaves.items()}


def main():
    g13, g14 = load_golden('g13_lora.npz'), load_golden('g14_lora_grad.npz')
    cu, ml = g14['cu_lens'], int(g14['max_len'])
    L, E, seed = (int(g13[f'esm2_{k}']) for k in ('L', 'E', 'seed'))
    args = (g14['esm2_tokens_in'], g14['esm2_tokens'], g14['esm2_mask'], cu, ml)
    lens = (cu[1:] - cu[:-1]).long()
    out = {'L': np.int32(L), 'E': np.int32(E), 'H': np.int32(HEADS), 'seed': np.int32(seed)}
    for kind in KINDS:
        weights = syn.synthetic_state_dict(kind, L, E, seed)
        loss64, g64 = step(weights, HEADS, torch.float64, *args)
        loss16, g16 = step(weights, HEADS, torch.bfloat16, *args)
        rows = ml + 2
        assert not bool(g64[POS][rows:].any()) and not bool(g16[POS][rows:].any()) and not bool(g64[POS][:2].any())
        out[f'{kind}_oracle/loss'] = np.float64(loss64)
        out[f'{kind}_fan_in'] = np.array([0, 0] + [int((lens > p).sum()) for p in range(ml)], dtype=np.int32)
        for k in stored(kind):
            a64, a16 = (g[k][:rows] if k == POS else g[k] for g in (g64, g16))
            out[f'{kind}_oracle/{k}'] = a64.numpy()
            out[f'{kind}_bf16_error/{k}'] = np.float64(FG.rel(a16, a64))
        print(f'  {kind}: loss f64 {float(loss64):.8f}, bf16 {float(loss16):.5f}; bf16 against f64: '
              + ', '.join(f'{k} {float(out[f"{kind}_bf16_error/{k}"]):.4f}' for k in stored(kind)))
    path = os.path.join(HERE, 'g18_position_grad.npz')
    np.savez_compressed(path, **out)
    print(f'  g18_position_grad.npz {os.path.getsize(path) / 1024:8.1f} KiB; {ml + 2} rows of the position table, fan-in up to {int(lens.numel())}')
    assert os.path.getsize(path) < 1_000_000


if __name__ == '__main__':
    main()
