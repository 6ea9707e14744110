"""Train the learned-position table of an ESM-1b / ESM-1v checkpoint alone on a FASTA file of long proteins: the reference's
workflow/positional_emb experiment (the run that made its 4 096-position ESM-1b / ESM-1v files) without Lightning.

  python tools/position_finetune.py CHECKPOINT.safetensors PROTEINS.fasta [--max-positions 8192] [--steps 100] [--lr 1e-6]
                                    [--token-per-batch 50000] [--accumulate 1] [--mask-freq 0.15] [--alter-freq 0.1]
                                    [--checkpoint-layers] [--out TRAINED.safetensors]

Everything is frozen, model.mark_trainable(False, False, positions=True) opts the table in, --max-positions extends it first
(model.extend_positions: the old rows kept, the new rows zeros).  FASTA -> esme.data.MaskedFastaTokenDataset (token-budget batches,
packed, BERT-style corruption) -> model.forward_trainable -> esme.cross_entropy at the selected positions -> esme.optim.AdamW with
fp32 master weights, --accumulate micro-batches per step through opt.accumulate().  Prints the loss per step.  --out writes the whole
model with the checkpoint metadata ESM.from_pretrained reads, so the result loads like the checkpoint it came from.  The hot path is
this package's kernels: the packed lookup, the attention forward and backward, the GEMMs, the position-table gradient
(esme_hip_embed_positions_bwd) and the fused optimiser step."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'esm-efficient_amd')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('checkpoint')
    ap.add_argument('fasta')
    ap.add_argument('--max-positions', type=int, default=0, help='extend the position table to this many positions first (0: keep it)')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--lr', type=float, default=1e-6)
    ap.add_argument('--weight-decay', type=float, default=1e-2)
    ap.add_argument('--max-grad-norm', type=float, default=1.0)
    ap.add_argument('--token-per-batch', type=int, default=50_000)
    ap.add_argument('--accumulate', type=int, default=1, help='micro-batches per optimiser step')
    ap.add_argument('--max-len', type=int, default=None)
    ap.add_argument('--mask-freq', type=float, default=0.15)
    ap.add_argument('--alter-freq', type=float, default=0.1)
    ap.add_argument('--checkpoint-layers', action='store_true', help='keep only the layers\' inputs and recompute each layer in the backward')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--out', default='', help='write the trained model here (safetensors, loadable by ESM.from_pretrained)')
    args = ap.parse_args()
    import esme
    from esme import ESM, synthetic as syn
    from esme.data import MaskedFastaTokenDataset
    torch.manual_seed(args.seed)
    model = ESM.from_pretrained(args.checkpoint, device=args.device)
    if getattr(model, 'embed_positions', None) is None:
        raise SystemExit(f'{type(model).__name__} has no learned position table: this tool serves ESM-1b / ESM-1v checkpoints')
    if args.max_positions:
        model.extend_positions(args.max_positions)
    model.mark_trainable(False, False, positions=True).mark_lmhead(False).train()
    params = [p for p in model.parameters() if p.requires_grad]
    assert params == [model.embed_positions.weight]
    limit = model.embed_positions.max_positions
    max_len = limit if args.max_len is None else min(args.max_len, limit)
    print(f'{type(model).__name__}: the position table alone trains, {model.embed_positions.num_embeddings} rows x {model.embed_dim}; sequences up to {max_len} tokens')
    data = MaskedFastaTokenDataset(args.fasta, token_per_batch=args.token_per_batch, max_len=max_len, mask_freq=args.mask_freq,
                                   alter_freq=args.alter_freq, shuffle=True, random_state=args.seed, alphabet=model.alphabet)
    opt = esme.optim.AdamW(params, lr=args.lr, weight_decay=args.weight_decay, max_grad_norm=args.max_grad_norm)
    step = micro = 0
    losses = []
    while step < args.steps:
        for tokens, (cu_lens, batch_max_len), masked, mask in data.to_dataloader():     # (every pass draws a new corruption)
            if tokens.numel() == 0:
                continue
            dev = lambda t: t.to(args.device, non_blocking=True)
            logits = model.forward_trainable(dev(masked), (dev(cu_lens), batch_max_len), checkpoint_layers=args.checkpoint_layers)
            loss = esme.cross_entropy(logits, dev(tokens), dev(mask), alphabet=model.alphabet)
            (loss / args.accumulate).backward()
            opt.accumulate()                                                            # p.grad into the fp32 accumulator, p.grad = None
            losses.append(loss.detach())
            micro += 1
            if micro % args.accumulate:
                continue
            opt.step()
            step += 1
            print(f'step {step:5d}  micro-batches {len(losses)}  rows {tokens.numel():6d}  loss {float(torch.stack(losses).mean()):.4f}  '
                  f'grad norm {float(opt.last_grad_norm):.3f}')
            losses = []
            if step >= args.steps:
                break
    if args.out:
        from safetensors import safe_open
        from safetensors.torch import save_file
        with safe_open(args.checkpoint, framework='pt', device='cpu') as f:
            name = (f.metadata() or {}).get('name', type(model).__name__.lower())
        metadata = syn.checkpoint_metadata(name, len(model.layers), model.embed_dim, model.attention_heads)
        save_file({k: v.detach().contiguous() for k, v in model.state_dict().items()}, args.out, metadata)
        print(f'wrote {args.out} ({model.embed_positions.num_embeddings} position rows)')


if __name__ == '__main__':
    main()
