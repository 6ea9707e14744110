"""Supervised fine-tuning of a backbone and a regression head on labelled sequences: the reference's RegressionTrainer recipe (its
meltome, GB1 / AAV fitness and TF-classification experiments) without Lightning.

  python tools/regression_finetune.py CHECKPOINT.safetensors TRAIN.tsv VAL.tsv [--epochs 1] [--lr 1e-5] [--lr-head 1e-4]
                                      [--lora RANK | --unfreeze-top K] [--layers 10,20] [--head attention|mean]
                                      [--token-per-batch 50000] [--truncate-len N] [--checkpoint-layers] [--out-lora ADAPTERS.safetensors]

TSV lines are `sequence<TAB>label` (a first line whose label is not a number is taken for a header).  esme.data.LabeledDataset
(token-budget batches, packed) -> esme.trainer.RegressionModel: the backbone (frozen by default; `--lora RANK` trains adapters on
query / value / output, `--unfreeze-top K` the last K layers) with the raw outputs of `--layers` next to the final representation ->
BinaryLearnedAggregation (`--head mean`: ClsHead) of width embed_dim * (1 + number of layers) -> F.mse_loss(reduction='sum') ->
esme.optim.AdamW with the head at --lr-head and the backbone at --lr.  Prints the train loss per step and, per epoch, the validation
loss and Spearman's rank correlation.  On the hot path: the packed forward, the attention and pooling backwards, the weight-gradient
GEMM, the mean-pool backward and the fused optimiser step, all this package's kernels; no step waits for the device except to print."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'esm-efficient_amd')]


def read_tsv(path):
    seqs, labels = [], []
    with open(path) as f:
        for n, line in enumerate(f):
            parts = line.rstrip('\n').split('\t')
            if len(parts) < 2 or not parts[0]:
                continue
            try:
                y = float(parts[1])
            except ValueError:
                if n == 0:
                    continue                             # a header line
                raise ValueError(f'{path}:{n + 1}: label {parts[1]!r} is not a number')
            seqs.append(parts[0].strip())
            labels.append(y)
    if not seqs:
        raise ValueError(f'{path}: no `sequence<TAB>label` lines')
    return seqs, labels


def batch_to(batch, device):
    dev = lambda t: t.to(device, non_blocking=True)
    return dev(batch['token']), (dev(batch['cu_lens']), int(batch['max_len'])), dev(batch['label'])


def validate(net, data, device):
    from esme.trainer import spearman
    net.eval()
    total, preds, labels = 0.0, [], []
    for batch in data.to_dataloader():
        if batch['token'].numel() == 0:
            continue
        token, pad_args, label = batch_to(batch, device)
        y = net(token, pad_args).float().reshape(-1)
        total += float(F.mse_loss(y, label, reduction='sum'))
        preds.append(y.cpu())
        labels.append(label.cpu())
    preds, labels = torch.cat(preds), torch.cat(labels)
    return total / labels.numel(), spearman(preds, labels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('checkpoint')
    ap.add_argument('train_tsv')
    ap.add_argument('val_tsv')
    ap.add_argument('--epochs', type=int, default=1)
    ap.add_argument('--lr', type=float, default=1e-5, help='the backbone\'s learning rate')
    ap.add_argument('--lr-head', type=float, default=1e-4)
    ap.add_argument('--weight-decay', type=float, default=1e-2)
    ap.add_argument('--max-grad-norm', type=float, default=None)
    group = ap.add_mutually_exclusive_group()
    group.add_argument('--lora', type=int, default=0, metavar='RANK', help='train LoRA adapters of this rank on query / value / output')
    group.add_argument('--unfreeze-top', type=int, default=0, metavar='K', help='train the projections and LayerNorms of the last K layers')
    ap.add_argument('--layers', default='', help='comma-separated layers whose raw outputs the head sees next to the final representation')
    ap.add_argument('--head', choices=('attention', 'mean'), default='attention')
    ap.add_argument('--head-heads', type=int, default=None, help='attention heads of the pooling head (default: the backbone\'s)')
    ap.add_argument('--token-per-batch', type=int, default=50_000)
    ap.add_argument('--truncate-len', type=int, default=None)
    ap.add_argument('--checkpoint-layers', action='store_true', help='keep only the layers\' inputs and recompute each layer in the backward')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--out-lora', default='', help='write the trained adapters here (model.save_lora)')
    args = ap.parse_args()
    import esme
    from esme import ESM
    from esme.data import LabeledDataset
    from esme.head import ClsHead
    from esme.pooling import BinaryLearnedAggregation
    from esme.trainer import RegressionModel
    torch.manual_seed(args.seed)
    model = ESM.from_pretrained(args.checkpoint, device=args.device)
    for p in model.parameters():
        p.requires_grad_(False)
    if args.lora:
        model.add_lora(rank=args.lora, alpha=args.lora, layers=('query', 'value', 'output'))
        model.mark_only_lora_as_trainable()
    elif args.unfreeze_top:
        model.mark_trainable(layers=range(-args.unfreeze_top, 0))
    layers = [int(i) for i in args.layers.split(',') if i.strip()]
    width = model.embed_dim * (1 + len(layers))
    if args.head == 'attention':
        head = BinaryLearnedAggregation(args.head_heads or model.attention_heads, width)
    else:
        head = ClsHead(width)
    head = head.to(args.device).requires_grad_(True)
    net = RegressionModel(model, head, layers=layers)
    opt = esme.optim.AdamW(net.param_groups(args.lr, args.lr_head), weight_decay=args.weight_decay, max_grad_norm=args.max_grad_norm)
    n_head, n_plm = (sum(p.numel() for p in m.parameters() if p.requires_grad) for m in (head, model))
    print(f'{type(model).__name__} + {type(head).__name__} of width {width}: {n_head / 1e6:.2f} M head and {n_plm / 1e6:.2f} M backbone parameters train')
    val = LabeledDataset(*read_tsv(args.val_tsv), args.token_per_batch, shuffle=False, truncate_len=args.truncate_len)
    seqs, labels = read_tsv(args.train_tsv)
    step = 0
    for epoch in range(args.epochs):
        data = LabeledDataset(seqs, labels, args.token_per_batch, shuffle=True, random_state=args.seed + epoch, truncate_len=args.truncate_len)
        net.train()
        for batch in data.to_dataloader():
            if batch['token'].numel() == 0:
                continue
            token, pad_args, label = batch_to(batch, args.device)
            net.zero_grad(set_to_none=True)
            y = net.forward_trainable(token, pad_args, checkpoint_layers=args.checkpoint_layers)
            loss = F.mse_loss(y.float().reshape(-1), label, reduction='sum')
            loss.backward()
            opt.step()
            step += 1
            print(f'epoch {epoch}  step {step:5d}  sequences {label.numel():4d}  rows {token.numel():6d}  loss {float(loss):.4f}')
        val_loss, rho = validate(net, val, args.device)
        print(f'epoch {epoch}  validation: mse {val_loss:.5f}  spearman {rho:.4f}')
    if args.out_lora and args.lora:
        model.save_lora(args.out_lora)
        print(f'wrote {args.out_lora}')


if __name__ == '__main__':
    main()
