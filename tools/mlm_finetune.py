"""Masked-LM training (continued pretraining) of every parameter on a FASTA file: the reference README's "Training the model"
section without Lightning.

  python tools/mlm_finetune.py CHECKPOINT.safetensors PROTEINS.fasta [--steps 100] [--lr 1e-4] [--token-per-batch 50000]
                               [--mask-freq 0.15] [--alter-freq 0.1] [--checkpoint-layers] [--out TRAINED.safetensors]

FASTA -> esme.data.MaskedFastaTokenDataset (token-budget batches, packed, BERT-style corruption by esme.alphabet.mask_tokens) ->
model.mark_trainable(embedding=True) + mark_lmhead() -> model.forward_trainable -> esme.cross_entropy at the selected positions ->
esme.optim.AdamW (fp32 master weights).  Prints the loss per step.  Everything on the hot path is this package's kernels: the packed
forward, the attention backward, the weight-gradient GEMM, the token-embedding gradient and the fused optimiser step."""
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
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--lr', type=float, default=1e-4)
    ap.add_argument('--weight-decay', type=float, default=1e-2)
    ap.add_argument('--max-grad-norm', type=float, default=1.0)
    ap.add_argument('--token-per-batch', type=int, default=50_000)
    ap.add_argument('--max-len', type=int, default=None)
    ap.add_argument('--mask-freq', type=float, default=0.15)
    ap.add_argument('--alter-freq', type=float, default=0.1)
    ap.add_argument('--checkpoint-layers', action='store_true', help='keep only the layers\' inputs and recompute each layer in the backward')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--out', default='', help='write the trained state_dict here (safetensors)')
    args = ap.parse_args()
    import esme
    from esme import ESM
    from esme.data import MaskedFastaTokenDataset
    torch.manual_seed(args.seed)
    model = ESM.from_pretrained(args.checkpoint, device=args.device)
    model.mark_trainable(embedding=True).mark_lmhead().train()
    params = [p for p in model.parameters() if p.requires_grad]
    print(f'{type(model).__name__}: {len(params)} tensors, {sum(p.numel() for p in params) / 1e6:.1f} M parameters train')
    data = MaskedFastaTokenDataset(args.fasta, token_per_batch=args.token_per_batch, max_len=args.max_len, mask_freq=args.mask_freq,
                                   alter_freq=args.alter_freq, shuffle=True, random_state=args.seed, alphabet=model.alphabet)
    opt = esme.optim.AdamW(params, lr=args.lr, weight_decay=args.weight_decay, max_grad_norm=args.max_grad_norm)
    step = 0
    while step < args.steps:
        for tokens, (cu_lens, max_len), masked, mask in data.to_dataloader():     # (every pass draws a new corruption)
            if tokens.numel() == 0:
                continue
            dev = lambda t: t.to(args.device, non_blocking=True)
            model.zero_grad(set_to_none=True)
            logits = model.forward_trainable(dev(masked), (dev(cu_lens), max_len), checkpoint_layers=args.checkpoint_layers)
            loss = esme.cross_entropy(logits, dev(tokens), dev(mask), alphabet=model.alphabet)
            loss.backward()
            opt.step()
            step += 1
            print(f'step {step:5d}  rows {tokens.numel():6d}  selected {int(mask.sum()):5d}  loss {float(loss):.4f}  grad norm {float(opt.last_grad_norm):.3f}')
            if step >= args.steps:
                break
    if args.out:
        from safetensors import safe_open
        from safetensors.torch import save_file
        with safe_open(args.checkpoint, framework='pt', device='cpu') as f:       # the geometry strings from_pretrained reads
            metadata = f.metadata() or {}
        save_file({k: v.detach().contiguous() for k, v in model.state_dict().items()}, args.out, metadata)
        print(f'wrote {args.out}')


if __name__ == '__main__':
    main()
