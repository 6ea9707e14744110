#!/usr/bin/env python
"""Golden fixture for esme.data.LabeledDataset: what the REFERENCE's LabeledDataset yields on the CPU.

    python tests/golden/make_golden_labeled_dataset.py     # rewrites g16_labeled_dataset.json

Runs only where make_golden.py runs (it imports the reference package through that script's flash_attn stand-in; the reference's
data module also imports `lightning` for its data modules and, through its FASTA reader, `polars`; where they are not installed
this script puts empty stand-ins in their place: the dataset class uses none of them).  40 sequences of lengths 1 .. 40 (random
residues, numpy PCG64) with one label each; per case -- two token budgets x shuffle off / on with a seed x truncate_len unset / set -- every item of the dataset: the batch's sequence numbers (`members`) and
the item's `token`, `cu_lens`, `max_len`, `indices` and `label`.  Data only.
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG                                 # noqa: E402

RESIDUES = 'ACDEFGHIKLMNPQRSTVWY'
BUDGETS = (64, 200)
SHUFFLES = ((False, None), (True, 3))
TRUNCATE = (None, 16)
SEED = 160


def lightning_stand_in():
    """The names the reference's data module needs at import time (base classes, the FASTA reader's table library); nothing of them is
    used by LabeledDataset."""
    top, pt, cb = types.ModuleType('lightning'), types.ModuleType('lightning.pytorch'), types.ModuleType('lightning.pytorch.callbacks')
    top.LightningDataModule, cb.Callback = object, object
    top.pytorch, pt.callbacks = pt, cb
    placed = []
    for m in (top, pt, cb, types.ModuleType('polars')):
        try:
            __import__(m.__name__)
        except ImportError:
            sys.modules[m.__name__] = m
            placed.append(m.__name__)
    return placed


def sequences():
    rng = np.random.Generator(np.random.PCG64(SEED))
    seqs = [''.join(RESIDUES[i] for i in rng.integers(0, len(RESIDUES), n)) for n in range(1, 41)]
    order = rng.permutation(len(seqs))                   # (not sorted by length: a greedy packer sees long and short ones mixed)
    seqs = [seqs[i] for i in order]
    labels = [float(np.float32(x)) for x in rng.standard_normal(len(seqs))]
    return seqs, labels


def main():
    MG.import_reference()
    placed = lightning_stand_in()
    from esme.data import LabeledDataset                 # (the reference's: `esme` is the reference package in this process)
    for name in placed:                                  # (scikit-learn's shuffle asks sys.modules for a real polars)
        del sys.modules[name]
    seqs, labels = sequences()
    cases = []
    for budget in BUDGETS:
        for shuffle, seed in SHUFFLES:
            for trunc in TRUNCATE:
                ds = LabeledDataset(seqs, labels, budget, shuffle=shuffle, random_state=seed, truncate_len=trunc)
                items = []
                for i in range(len(ds)):
                    it = ds[i]
                    items.append({'members': [int(j) for j in ds.sampler[i]], 'token': it['token'].tolist(), 'cu_lens': it['cu_lens'].tolist(),
                                  'max_len': int(it['max_len']), 'indices': it['indices'].tolist(), 'label': [float(x) for x in it['label']]})
                cases.append({'token_per_batch': budget, 'shuffle': shuffle, 'random_state': seed, 'truncate_len': trunc, 'items': items})
                print(f'  budget {budget}, shuffle {shuffle}, truncate_len {trunc}: {len(items)} batches')
    path = os.path.join(HERE, 'g16_labeled_dataset.json')
    with open(path, 'w') as f:
        json.dump({'seqs': seqs, 'labels': labels, 'cases': cases}, f, separators=(',', ':'))
    print(f'  g16_labeled_dataset.json {os.path.getsize(path) / 1024:8.1f} KiB')
    assert os.path.getsize(path) < 1_000_000


if __name__ == '__main__':
    main()
