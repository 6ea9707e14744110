"""Per-residue fine-tuning: LoRA adapters on a backbone and a ResidueHead trained for a label per residue, the packed counterpart of
Hugging Face's EsmForTokenClassification recipe.

  python tools/residue_finetune.py [CHECKPOINT.safetensors] [--steps 200] [--lora 8] [--lr 3e-3] [--lr-head 1e-2] [--layers 0]
                                   [--token-per-batch 4000] [--sequences 256] [--checkpoint-layers] [--crf] [--out FILE]

Without a checkpoint a small synthetic ESM-2 (--synthetic-layers x --synthetic-dim) is used.  The task is synthetic and computable
from the sequence, so the tool needs no data: the label of residue i is the class of the residue two positions on -- hydrophobic (0),
polar (1) or charged (2) -- and the last two residues of a protein carry no label (they are negative, hence ignored, like `<cls>` and
`<eos>`).  A head over a single row cannot solve it: the backbone's attention has to carry the neighbour's identity over, which is what
the adapters learn.  esme.data.ResidueLabeledDataset (token-budget batches, labels aligned with the packed tokens) ->
esme.trainer.ResidueModel.loss_trainable: forward_trainable(logits=False, layers=...) -> ResidueHead.loss, the fused projection +
cross-entropy kernel (include/esme_hip_linear_xent.h) -> esme.optim.AdamW.  Prints the loss per step and the final per-residue
accuracy.  --crf puts a linear-chain CRF on the head (esme.head.ResidueCRFHead, include/esme_hip_crf.h) and changes the task to one with a
rule between neighbouring labels (make_segment_task): the loss is the CRF's negative log-likelihood, the prediction the Viterbi path.
No step waits for the device except to print: the loss is a device scalar and is read after the optimiser step was queued."""
import argparse
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'esm-efficient_amd')]

HYDROPHOBIC, POLAR, CHARGED = 'AVLIMFWCGP', 'STNQYH', 'DEKR'
RESIDUES = HYDROPHOBIC + POLAR + CHARGED
CLASS_OF = {**{r: 0 for r in HYDROPHOBIC}, **{r: 1 for r in POLAR}, **{r: 2 for r in CHARGED}}
SHIFT = 2


def make_task(n_seq, seed=0, lo=20, hi=120):
    """(sequences, labels): random proteins of lo .. hi residues; labels[i][j] = the class of residue j + SHIFT, -1 on the last SHIFT."""
    g = torch.Generator().manual_seed(seed)
    seqs, labels = [], []
    for _ in range(n_seq):
        n = int(torch.randint(lo, hi + 1, (1,), generator=g))
        s = ''.join(RESIDUES[i] for i in torch.randint(0, len(RESIDUES), (n,), generator=g).tolist())
        seqs.append(s)
        labels.append([CLASS_OF[c] for c in s[SHIFT:]] + [-1] * SHIFT)
    return seqs, labels


def make_segment_task(n_seq, seed=0, lo=20, hi=120, run=4):
    """(sequences, labels) with a rule between neighbouring labels that no single row shows: a charged residue opens a segment of
    label 1 that lasts exactly `run` residues, everything else is label 0 -- so 0 -> 1 only at a charged residue and 1 -> 0 only after
    `run` ones; label 2 marks the last residue of a segment (1 -> 2 -> 0).  The residues inside a segment are random."""
    g = torch.Generator().manual_seed(seed)
    seqs, labels = [], []
    for _ in range(n_seq):
        n = int(torch.randint(lo, hi + 1, (1,), generator=g))
        s = ''.join(RESIDUES[i] for i in torch.randint(0, len(RESIDUES), (n,), generator=g).tolist())
        lab, left = [], 0
        for c in s:
            if left == 0 and c in CHARGED:
                left = run
            lab.append(0 if left == 0 else (2 if left == 1 else 1))
            left = max(left - 1, 0)
        seqs.append(s)
        labels.append(lab)
    return seqs, labels


def batch_to(batch, device):
    dev = lambda t: t.to(device, non_blocking=True)
    return dev(batch['token']), (dev(batch['cu_lens']), int(batch['max_len'])), dev(batch['label'])


def train_steps(net, opt, batches, device, steps, checkpoint_layers=False, log=None):
    """`steps` optimiser steps over `batches` (cycled): the list of the losses, read from the device after each step was queued."""
    losses, step = [], 0
    net.train()
    while step < steps:
        for batch in batches:
            if step >= steps:
                break
            if batch['token'].numel() == 0:
                continue
            token, pad_args, label = batch_to(batch, device)
            net.zero_grad(set_to_none=True)
            loss = net.loss_trainable(token, pad_args, label, checkpoint_layers=checkpoint_layers)
            loss.backward()
            opt.step()
            step += 1
            losses.append(float(loss.detach()))
            if log is not None:
                log(f'step {step:4d}  rows {token.numel():6d}  loss {losses[-1]:.4f}')
    return losses


def accuracy(net, batches, device):
    """The share of the labelled residues whose argmax label is right."""
    net.eval()
    right = total = 0
    for batch in batches:
        if batch['token'].numel() == 0:
            continue
        token, pad_args, label = batch_to(batch, device)
        pred = net.predict(token, pad_args)
        keep = label >= 0
        right += int((pred[keep] == label[keep]).sum())
        total += int(keep.sum())
    return right / max(total, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('checkpoint', nargs='?', default='')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--lora', type=int, default=8, metavar='RANK')
    ap.add_argument('--lr', type=float, default=3e-3, help='the adapters\' learning rate')
    ap.add_argument('--lr-head', type=float, default=1e-2)
    ap.add_argument('--weight-decay', type=float, default=0.0)
    ap.add_argument('--layers', default='0', help='comma-separated layers whose raw outputs the head sees next to the final representation')
    ap.add_argument('--token-per-batch', type=int, default=4000)
    ap.add_argument('--sequences', type=int, default=256)
    ap.add_argument('--synthetic-layers', type=int, default=2)
    ap.add_argument('--synthetic-dim', type=int, default=128)
    ap.add_argument('--checkpoint-layers', action='store_true')
    ap.add_argument('--crf', action='store_true', help='a linear-chain CRF on the head, and the segment task')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--out', default='', help='append the printed lines to this file')
    args = ap.parse_args()
    import esme
    from esme import ESM, synthetic as syn
    from esme.data import ResidueLabeledDataset
    from esme.head import ResidueCRFHead, ResidueHead
    from esme.trainer import ResidueModel
    torch.manual_seed(args.seed)
    lines = []

    def log(s):
        print(s)
        lines.append(s)
    if args.checkpoint:
        model = ESM.from_pretrained(args.checkpoint, device=args.device)
    else:
        with tempfile.TemporaryDirectory() as td:
            path = syn.write_checkpoint(os.path.join(td, 'm.safetensors'), 'esm2_t', args.synthetic_layers, args.synthetic_dim,
                                        args.synthetic_dim // 64, seed=args.seed)
            model = ESM.from_pretrained(path, device=args.device)
    for p in model.parameters():
        p.requires_grad_(False)
    model.add_lora(rank=args.lora, alpha=args.lora, layers=('query', 'value', 'output'))
    model.mark_only_lora_as_trainable()
    layers = [int(i) for i in args.layers.split(',') if i.strip()]
    head = (ResidueCRFHead if args.crf else ResidueHead)(model.embed_dim * (1 + len(layers)), 3).to(args.device).requires_grad_(True)
    net = ResidueModel(model, head, layers=layers)
    opt = esme.optim.AdamW(net.param_groups(args.lr, args.lr_head), weight_decay=args.weight_decay)
    n_head, n_plm = (sum(p.numel() for p in m.parameters() if p.requires_grad) for m in (head, model))
    task = make_segment_task if args.crf else make_task
    what = 'segments of four residues opened by a charged residue' if args.crf else f'label of residue i = class (hydrophobic / polar / charged) of residue i + {SHIFT}'
    log(f'{type(model).__name__} ({len(model.layers)} layers, width {model.embed_dim}) + {type(head).__name__} of width {net.width}: {n_head} head and '
        f'{n_plm} adapter parameters train; {what}')
    seqs, labels = task(args.sequences, args.seed)
    data = ResidueLabeledDataset(seqs, labels, args.token_per_batch, shuffle=True, random_state=args.seed)
    batches = [data[i] for i in range(len(data))]
    held = ResidueLabeledDataset(*task(max(args.sequences // 4, 8), args.seed + 1), args.token_per_batch, shuffle=False)
    held = [held[i] for i in range(len(held))]
    log(f'accuracy before training: {accuracy(net, held, args.device):.4f} on held-out proteins (three classes)')
    train_steps(net, opt, batches, args.device, args.steps, args.checkpoint_layers, log)
    log(f'accuracy after {args.steps} steps: {accuracy(net, held, args.device):.4f} on held-out proteins, {accuracy(net, batches, args.device):.4f} on the training set')
    if args.out:
        with open(args.out, 'a') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
