#!/usr/bin/env python
"""Golden fixture for esme.alphabet.mask_tokens: what the REFERENCE's mask_tokens returns, for three seeds.

    python tests/golden/make_golden_mask_tokens.py     # rewrites g16_mask_tokens.npz

Runs only where make_golden.py runs (it imports the reference package through that script's flash_attn stand-in).  Bit-equality with
the reference's random stream is not a goal of this project's mask_tokens, so the file is not compared with its output: the property
checker of tests/test_embed_bwd_cpu.py (special tokens untouched, a selection in every row, the selected share and the three outcome
shares within 5 binomial standard deviations) runs over the reference's own output recorded here, which validates the checker.

Per seed s: `s{s}_tokens` (int8), `s{s}_masked` (int8), `s{s}_mask` (bool) -- two 2-D padded batches and one 1-D packed batch of random
residues between `<cls>` and `<eos>` -- and the scalars `freq`, `alter`.  Data only.
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG                                 # noqa: E402

FREQ, ALTER = 0.15, 0.1
SEEDS = (0, 1, 2)


def batch(seed, packed, alphabet):
    g = torch.Generator().manual_seed(100 + seed)
    lens = torch.randint(30, 400, (96,), generator=g).tolist()
    rows = [torch.cat((torch.tensor([alphabet.cls_idx]), torch.randint(4, 24, (n,), generator=g), torch.tensor([alphabet.eos_idx]))) for n in lens]
    if packed:
        return torch.cat(rows)
    out = torch.full((len(rows), max(lens) + 2), alphabet.padding_idx, dtype=torch.int64)
    for i, r in enumerate(rows):
        out[i, :r.numel()] = r
    return out


def main():
    ref = MG.import_reference()
    from esme.alphabet import Alphabet3, mask_tokens     # (the reference's: `esme` is the reference package in this process)
    data = {'freq': np.float64(FREQ), 'alter': np.float64(ALTER)}
    for s in SEEDS:
        tokens = batch(s, packed=(s == 2), alphabet=Alphabet3)
        torch.manual_seed(s)
        masked, mask = mask_tokens(tokens, FREQ, ALTER, alphabet=Alphabet3)
        data[f's{s}_tokens'], data[f's{s}_masked'], data[f's{s}_mask'] = tokens.numpy().astype(np.int8), masked.numpy().astype(np.int8), mask.numpy()
        print(f'  seed {s}: {tuple(tokens.shape)}, {int(mask.sum())} selected')
    path = os.path.join(HERE, 'g16_mask_tokens.npz')
    np.savez_compressed(path, **data)
    print(f'  g16_mask_tokens.npz {os.path.getsize(path) / 1024:8.1f} KiB')
    assert os.path.getsize(path) < 1_000_000


if __name__ == '__main__':
    main()
