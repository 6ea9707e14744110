"""Token-budget batching of a FASTA file into packed forward inputs.

The caller side of the hot path: `FastaTokenDataset[i]` is exactly the
`(tokens, (cu_lens, max_len))` pair `ESM2.forward` consumes.  Names, arguments and the
greedy packing rule follow `esme/data.py:12-60,63-162` of the reference.  `MaskedFastaDataset` /
`MaskedFastaTokenDataset` add the masked-token corruption of `esme.alphabet.mask_tokens` for
masked-LM training (the reference's constructor arguments and item layouts, data.py:165-245);
`LabeledDataset` pairs in-memory sequences with one label each for supervised fine-tuning (esme.trainer.RegressionModel; the
reference's constructor arguments and item dict, data.py:377-407) and `ResidueLabeledDataset` with one label per residue
(esme.trainer.ResidueModel); the Lightning data modules (data.py:247-374, 410-520:
MaskedFastaDataModule, LabeledDataModule) stay out of scope.
"""
from __future__ import annotations

from typing import List, Sequence

from torch.utils.data import DataLoader, Dataset

import torch
from esme.alphabet import Alphabet3, mask_tokens, pad_tokens, tokenize, tokenize_unpad
from esme.fasta import Fasta


class TokenSizeBatchSampler:
    """Greedy batches of sequence indices whose token count (length + 2 for cls/eos) stays
    within `token_per_batch`.  Walks the (optionally shuffled) order once; a batch is closed
    when the next sequence would overflow it.  Like the reference (data.py:33-54) a sequence
    longer than the whole budget still gets a batch of its own, and if the very first one
    overflows, the first batch emitted is empty."""

    def __init__(self, token_sizes: Sequence[int], token_per_batch: int, drop_last: bool = False,
                 shuffle: bool = True, random_state=None):
        self.token_sizes = token_sizes
        self.token_per_batch = token_per_batch
        self.drop_last, self.shuffle, self.random_state = drop_last, shuffle, random_state
        self._batches = list(self.batches())

    def batches(self):
        order: List[int] = list(range(len(self.token_sizes)))
        if self.shuffle:
            import sklearn.utils            # the reference's shuffle, so seeds give the same order
            order = sklearn.utils.shuffle(order, random_state=self.random_state)
        batch, used = [], 0
        for idx in order:
            need = self.token_sizes[idx] + 2
            if used + need > self.token_per_batch:
                yield batch
                batch, used = [idx], need
            else:
                batch.append(idx)
                used += need
        if batch and not self.drop_last:
            yield batch

    def __iter__(self):
        return iter(self._batches)

    def __getitem__(self, idx):
        return self._batches[idx]

    def __len__(self):
        return len(self._batches)


class BaseFastaDataset(Dataset):
    def __init__(self, fasta, fai=None, k_sample=None, max_len=None, alphabet=Alphabet3):
        self.max_len = max_len or float('inf')
        self.alphabet = alphabet
        self.fasta = Fasta(fasta, fai=fai, max_len=max_len, k_sample=k_sample)

    def read_seq(self, idx):
        return self.fasta[idx]


class FastaDataset(BaseFastaDataset):
    """One tokenised sequence per item; `collate_fn` right-pads a batch (data.py:82-112)."""

    def __len__(self):
        return len(self.fasta)

    def __getitem__(self, idx):
        return tokenize(self.read_seq(idx), alphabet=self.alphabet)

    def collate_fn(self, batch):
        return pad_tokens(batch, alphabet=self.alphabet)

    def to_dataloader(self, batch_size, shuffle=False, num_workers=0, **kwargs):
        return DataLoader(self, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers,
                          collate_fn=self.collate_fn, **kwargs)


class FastaTokenDataset(BaseFastaDataset):
    """Item i = the i-th token-budget batch, already packed: `(tokens, (cu_lens, max_len))`
    (data.py:115-162)."""

    def __init__(self, fasta, fai=None, token_per_batch=50_000, k_sample=None, max_len=None,
                 drop_last=False, shuffle=True, random_state=None, alphabet=Alphabet3):
        super().__init__(fasta, fai=fai, k_sample=k_sample, max_len=max_len, alphabet=alphabet)
        self.token_per_batch = token_per_batch
        lengths = [row['length'] for row in self.fasta.fai]
        self.sampler = list(TokenSizeBatchSampler(lengths, token_per_batch, drop_last=drop_last,
                                                  shuffle=shuffle, random_state=random_state))

    def __len__(self):
        return len(self.sampler)

    def __getitem__(self, idx):
        token, _, cu_lens, max_len = tokenize_unpad([self.read_seq(i) for i in self.sampler[idx]],
                                                    alphabet=self.alphabet)
        return token, (cu_lens, max_len)

    def to_dataloader(self, num_workers=0, **kwargs):
        """One packed batch per item (batch_size=None).  On one GPU keep `num_workers=0`: an item takes ~20 ms of one core against 60 - 70 ms of GPU time
        for it, while worker processes FORKED from a process that already holds a GPU context stall its queues for 1 - 3 s when they start
        (profiles/r05_e2e_fork_stall.txt); pass `multiprocessing_context='forkserver'` if workers are needed."""
        return DataLoader(self, num_workers=num_workers, batch_size=None, **kwargs)


class MaskedFastaDataset(FastaDataset):
    """One sequence per item with its masked-token corruption: `(tokens, masked_tokens, mask)`, each (1, L); `collate_fn` right-pads a
    batch (`<pad>` for the ids, False for the mask).  `mask_freq` / `alter_freq`: `freq` / `alter` of esme.alphabet.mask_tokens."""

    def __init__(self, fasta, fai=None, max_len=None, k_sample=None, mask_freq=.15, alter_freq=.1, alphabet=Alphabet3):
        super().__init__(fasta, fai=fai, k_sample=k_sample, max_len=max_len, alphabet=alphabet)
        self.mask_freq, self.alter_freq = mask_freq, alter_freq

    def __getitem__(self, idx):
        token = super().__getitem__(idx)
        masked, mask = mask_tokens(token, self.mask_freq, self.alter_freq, alphabet=self.alphabet)
        return token, masked, mask

    def collate_fn(self, batch):
        tokens = pad_tokens([b[0] for b in batch], alphabet=self.alphabet)
        masked = pad_tokens([b[1] for b in batch], alphabet=self.alphabet)
        mask = torch.zeros(tokens.shape, dtype=torch.bool)
        for i, b in enumerate(batch):
            mask[i, :b[2].numel()] = b[2].reshape(-1)
        return tokens, masked, mask


class MaskedFastaTokenDataset(FastaTokenDataset):
    """Item i = the i-th token-budget batch, packed, with its masked-token corruption:
    `(tokens, (cu_lens, max_len), masked_tokens, mask)` -- `masked_tokens` is the model's input, `tokens[mask]` the targets."""

    def __init__(self, fasta, fai=None, token_per_batch=50_000, k_sample=None, max_len=None, mask_freq=.15, alter_freq=.1,
                 drop_last=False, shuffle=True, random_state=None, alphabet=Alphabet3):
        super().__init__(fasta, fai=fai, token_per_batch=token_per_batch, k_sample=k_sample, max_len=max_len, drop_last=drop_last,
                         shuffle=shuffle, random_state=random_state, alphabet=alphabet)
        self.mask_freq, self.alter_freq = mask_freq, alter_freq

    def __getitem__(self, idx):
        tokens, unpad_args = super().__getitem__(idx)
        masked, mask = mask_tokens(tokens, self.mask_freq, self.alter_freq, alphabet=self.alphabet)
        return tokens, unpad_args, masked, mask


class LabeledDataset(Dataset):
    """Item i = the i-th token-budget batch of in-memory sequences with one number each, as a dict: `token`, `cu_lens`, `max_len`,
    `indices` (what tokenize_unpad returns for the batch's sequences) and `label`, a float32 tensor in batch order.  The batches are
    TokenSizeBatchSampler's over the sequences' FULL lengths; `truncate_len` cuts what is tokenised to its first `truncate_len`
    residues, not what is budgeted (so a truncated batch is below its budget, as in the reference)."""

    def __init__(self, seqs, labels, token_per_batch, shuffle=True, random_state=None, truncate_len=None):
        if len(seqs) != len(labels):
            raise ValueError(f'LabeledDataset: {len(seqs)} sequences but {len(labels)} labels')
        self.seqs, self.labels, self.truncate_len = seqs, labels, truncate_len
        self.sampler = list(TokenSizeBatchSampler([len(s) for s in seqs], token_per_batch, shuffle=shuffle, random_state=random_state))

    def truncate(self, seq):
        return seq if self.truncate_len is None else seq[:self.truncate_len]

    def __len__(self):
        return len(self.sampler)

    def __getitem__(self, idx):
        batch = self.sampler[idx]
        token, indices, cu_lens, max_len = tokenize_unpad([self.truncate(self.seqs[i]) for i in batch])
        label = torch.tensor([float(self.labels[i]) for i in batch], dtype=torch.float32)
        return {'token': token, 'cu_lens': cu_lens, 'max_len': max_len, 'indices': indices, 'label': label}

    def to_dataloader(self, num_workers=0, **kwargs):
        """One packed batch per item (batch_size=None); see FastaTokenDataset.to_dataloader on `num_workers`."""
        return DataLoader(self, num_workers=num_workers, batch_size=None, **kwargs)


class ResidueLabeledDataset(Dataset):
    """Item i = the i-th token-budget batch of in-memory sequences with one label per residue, as LabeledDataset's dict (`token`,
    `cu_lens`, `max_len`, `indices`: the same sampler, hence the same batches for the same seed) with `label` an int64 tensor (T,)
    aligned with the packed `token`: `ignore_index` on the `<cls>` / `<eos>` rows and wherever the user's label is negative, the
    user's integer elsewhere -- what esme.head.ResidueHead.loss takes.

    labels[i]: a sequence of len(seqs[i]) integers, or with `classes` (e.g. 'HEC') a string of that length whose characters map to
    their position in `classes`; any other character maps to `ignore_index`.  A label sequence whose length differs from its
    protein's is a ValueError here, at construction.  `truncate_len` cuts sequence and labels alike (the budget is taken over the full
    lengths, as in LabeledDataset)."""

    def __init__(self, seqs, labels, token_per_batch, shuffle=True, random_state=None, truncate_len=None, classes=None, ignore_index=-100):
        if len(seqs) != len(labels):
            raise ValueError(f'ResidueLabeledDataset: {len(seqs)} sequences but {len(labels)} label sequences')
        for i, (s, l) in enumerate(zip(seqs, labels)):
            if len(s) != len(l):
                raise ValueError(f'ResidueLabeledDataset: sequence {i} has {len(s)} residues but {len(l)} labels')
            if classes is not None and not isinstance(l, str):
                raise ValueError(f'ResidueLabeledDataset: classes={classes!r} maps label strings, but labels[{i}] is {type(l).__name__}')
        self.seqs, self.labels, self.truncate_len = seqs, labels, truncate_len
        self.classes, self.ignore_index = classes, int(ignore_index)
        self._class_of = None if classes is None else {ch: k for k, ch in enumerate(classes)}
        self.sampler = list(TokenSizeBatchSampler([len(s) for s in seqs], token_per_batch, shuffle=shuffle, random_state=random_state))

    def truncate(self, seq):
        return seq if self.truncate_len is None else seq[:self.truncate_len]

    def encode_labels(self, lab) -> torch.Tensor:
        """int64 (len(lab) + 2,): `ignore_index`, the (truncated) labels, `ignore_index`."""
        lab = self.truncate(lab)
        if self._class_of is not None:
            body = torch.tensor([self._class_of.get(ch, self.ignore_index) for ch in lab], dtype=torch.int64)
        else:
            body = torch.as_tensor([int(v) for v in lab], dtype=torch.int64).reshape(-1)
            body = torch.where(body < 0, torch.full_like(body, self.ignore_index), body)
        edge = torch.full((1,), self.ignore_index, dtype=torch.int64)
        return torch.cat((edge, body, edge))

    def __len__(self):
        return len(self.sampler)

    def __getitem__(self, idx):
        batch = self.sampler[idx]
        token, indices, cu_lens, max_len = tokenize_unpad([self.truncate(self.seqs[i]) for i in batch])
        label = torch.cat([self.encode_labels(self.labels[i]) for i in batch])
        if label.numel() != token.numel():
            raise ValueError(f'ResidueLabeledDataset: batch {idx} tokenises to {token.numel()} rows but carries {label.numel()} labels '
                             '(a sequence holds a multi-character token?)')
        return {'token': token, 'cu_lens': cu_lens, 'max_len': max_len, 'indices': indices, 'label': label}

    def to_dataloader(self, num_workers=0, **kwargs):
        """One packed batch per item (batch_size=None); see FastaTokenDataset.to_dataloader on `num_workers`."""
        return DataLoader(self, num_workers=num_workers, batch_size=None, **kwargs)
