"""What the contact regression's features cost: one esme_hip_contact_features call next to one esme_hip_contact_layer call on the same
operands, and model.contact_features next to a plain forward_representation.

  python tools/contact_features_bench.py [--reps 20] [--warmup 5] [--out profiles/contact_features_bench.txt]

Kernel cost: H = 15, d = 64 (ESM-C geometry), q / k column views of one random (T, 3E) bf16 buffer, sequences of S = 300 and S = 1 000
residues (plus bos / eos), 1 and 8 sequences per call, pairs = every i < j with j - i >= 6.  HIP events around each call, the median of
--reps calls after --warmup.  End to end: synthetic ESM-C 300M (30 layers, E = 960, H = 15), 8 x 300 and 2 x 1 000 residues, precision 'fast'.
There is no pass mark: the figures say what a fit costs, and whether a dense MFMA-tile variant of the gather pass would be worth building
(the gather pass moves 2 H d bf16 values per pair and side; contact_layer forms the same scores 64 x 64 at a time on the MFMA)."""
import argparse
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'esm-efficient_amd')]
DEV = 'cuda:0'


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def kernel_rows(S, B, H, d, warmup, reps):
    from esme import _hip, _hip_contact_features as HF, _hip_contacts as HC
    from esme.contacts import all_pairs
    rows, E = S + 2, H * d
    T = B * rows
    g = torch.Generator().manual_seed(S + B)
    qkv = (torch.randn(T, 3 * E, generator=g) * 1.2).to(torch.bfloat16).to(DEV)
    q, k = qkv[:, :E], qkv[:, E:2 * E]
    cu = torch.arange(0, T + 1, rows, dtype=torch.int32, device=DEV)
    pairs = all_pairs([S] * B, 6, DEV)
    feat = torch.empty(pairs.shape[0], H, dtype=torch.float32, device=DEV)
    n, off, total = HC.map_offsets(cu, 1, 1)
    out = torch.empty(total, dtype=torch.float32, device=DEV)
    w = torch.randn(H, generator=g).to(DEV)
    ws = torch.empty(HF.workspace_bytes(B, T, H), dtype=torch.uint8, device=DEV)
    scale = d ** -0.5
    with _hip.stream_scope(DEV):
        layer = timed(lambda: HC.contact_layer(q, k, cu, rows, H, d, scale, w, 0.0, True, out, off, ws), warmup, reps)
        feats = timed(lambda: HF.contact_features(q, k, cu, rows, H, d, scale, pairs, feat, 0, ws), warmup, reps)
    return (f'S {S:5d}  B {B}  pairs {pairs.shape[0]:9d}   contact_layer {layer[0] * 1e3:9.1f} us (min {layer[1] * 1e3:.1f}, max {layer[2] * 1e3:.1f})   '
            f'contact_features {feats[0] * 1e3:9.1f} us (min {feats[1] * 1e3:.1f}, max {feats[2] * 1e3:.1f})   ratio {feats[0] / layer[0]:.2f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    from esme import ESM, synthetic as syn
    lines = [f'device {torch.cuda.get_device_name(0)}; median of {args.reps} after {args.warmup} warm-ups, HIP events',
             'one esme_hip_contact_features call against one esme_hip_contact_layer call, H 15, d 64, pairs = every i < j with j - i >= 6:']
    for S in (300, 1000):
        for B in (1, 8):
            lines.append('  ' + kernel_rows(S, B, 15, 64, args.warmup, args.reps))
    with tempfile.TemporaryDirectory() as td:
        model = ESM.from_pretrained(syn.write_checkpoint(os.path.join(td, 'm.safetensors'), 'esmc_300m'), device=DEV)
    lines.append("model.contact_features (min_sep 6) against model.forward_representation, ESM-C 300M synthetic, precision 'fast':")
    with torch.no_grad():
        for total, S in ((8 * 302, 302), (2 * 1002, 1002)):
            tokens, cu, max_len, _ = syn.uniform_batch(total, S, seed=0)
            tokens, cu = tokens.to(DEV), cu.to(DEV)
            fw = timed(lambda: model.forward_representation(tokens, (cu, max_len)), args.warmup, args.reps)
            cf = timed(lambda: model.contact_features(tokens, (cu, max_len), min_sep=6), args.warmup, args.reps)
            X, pairs = model.contact_features(tokens, (cu, max_len), min_sep=6)
            lines.append(f'  {cu.numel() - 1} x {S - 2} residues, {pairs.shape[0]} pairs, X {tuple(X.shape)} = {X.numel() * 4 / 2 ** 20:.0f} MiB:   forward_representation '
                         f'{fw[0]:8.2f} ms   contact_features {cf[0]:8.2f} ms   ratio {cf[0] / fw[0]:.2f}   ({(cf[0] - fw[0]) / len(model.layers) * 1e3:.0f} us per layer)')
            del X, pairs
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
