"""Cost of the attention backward kernel (esme_hip_attn_varlen_bwd) next to the forward attention kernel, timed in the same run.

  python tools/attn_bwd_bench.py [--reps 20] [--warmup 5] [--out profiles/attn_bwd_bench.txt]

ESM2-650M's attention geometry (H = 20, d = 64) on 50 000 packed rows, bf16, random q / k / v / dO: (i) 100 sequences of 500 rows,
(ii) the proteome-like ragged batch of esme.synthetic.proteome_lengths.  HIP events around each call, the median of --reps calls
after --warmup.  Reported per batch:
  * the backward's time (its three launches: statistics + D, dK / dV, dQ);
  * its share of the bf16 MFMA peak over the flops it EXECUTES: nine S x S x d products per sequence and head (two score passes of
    the statistics kernel, S, dP, dV, dK in the dK / dV kernel, S, dP, dQ in the dQ kernel), 2 S^2 d flops each, tile padding not
    counted -- MFMA-bound by a wide margin (the operands of a 500-row sequence are re-read from L2), so the peak rate is the bound;
  * the ratio to the forward attention kernel (two products per sequence and head: the flop ratio is 4.5).
There is no pass mark: this first version buys run-to-run and batch-independent bits with seven products where an atomics-based
backward runs five, stages its transposed tiles through LDS with 2-byte stores and does not overlap loads with MFMAs.  The numbers
are what a later performance change starts from."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'esm-efficient_amd')]
PEAK_BF16_TFLOPS = 2500.0      # dense bf16 MFMA peak of the MI355X (bench.py uses the same figure)
BWD_PRODUCTS, FWD_PRODUCTS = 9, 2


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rows', type=int, default=50000)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    from esme import _hip, _hip_attn_bwd as HB, synthetic as syn
    dev, H, d = 'cuda:0', 20, 64
    E, scale = H * d, d ** -0.5
    lines = [f'attention backward, H = {H}, d = {d}, bf16, {args.rows} packed rows; median of {args.reps} calls after {args.warmup} warm-ups, HIP events',
             f'device {torch.cuda.get_device_name(0)}; peak taken as {PEAK_BF16_TFLOPS:.0f} TFLOP/s (dense bf16 MFMA)']
    batches = (('uniform, S = 500', syn.uniform_batch(args.rows, 500, seed=0)[1:3]),
               ('proteome-like ragged', syn.proteome_batch(args.rows, seed=0)[1:3]))
    for name, (cu, max_len) in batches:
        lens = (cu[1:] - cu[:-1]).double()
        T = int(cu[-1])
        g = torch.Generator().manual_seed(1)
        qkv = torch.randn(T, 3 * E, generator=g).to(torch.bfloat16).to(dev)
        d_o = torch.randn(T, E, generator=g).to(torch.bfloat16).to(dev)
        q, k, v = (qkv[:, i * E:(i + 1) * E] for i in range(3))
        cu = cu.to(dev)
        o = _hip.attn_varlen(q, k, v, cu, max_len, H, softmax_scale=scale)
        grads = torch.empty(T, 3 * E, dtype=torch.bfloat16, device=dev)
        dq, dk, dv = (grads[:, i * E:(i + 1) * E] for i in range(3))
        ws = torch.empty(HB.workspace_bytes(cu.numel() - 1, T, H), dtype=torch.uint8, device=dev)
        fwd = timed(lambda: _hip.attn_varlen(q, k, v, cu, max_len, H, softmax_scale=scale, out=o), args.warmup, args.reps)
        bwd = timed(lambda: HB.attn_varlen_bwd(q, k, v, o, d_o, cu, max_len, H, scale, dq, dk, dv, ws), args.warmup, args.reps)
        pair = 2.0 * float((lens * lens).sum()) * d * H              # flops of one S x S x d product over the batch
        tf_b, tf_f = BWD_PRODUCTS * pair / (bwd[0] * 1e-3) / 1e12, FWD_PRODUCTS * pair / (fwd[0] * 1e-3) / 1e12
        lines += [f'{name}: {cu.numel() - 1} sequences, longest {max_len}, {T} rows',
                  f'  backward {bwd[0]:8.3f} ms (min {bwd[1]:.3f}, max {bwd[2]:.3f})   {tf_b:7.1f} TFLOP/s executed = {100 * tf_b / PEAK_BF16_TFLOPS:5.2f} % of the bf16 MFMA peak',
                  f'  forward  {fwd[0]:8.3f} ms (min {fwd[1]:.3f}, max {fwd[2]:.3f})   {tf_f:7.1f} TFLOP/s executed = {100 * tf_f / PEAK_BF16_TFLOPS:5.2f} % of the bf16 MFMA peak',
                  f'  backward / forward = {bwd[0] / fwd[0]:.2f} in time ({BWD_PRODUCTS / FWD_PRODUCTS:.1f} in executed flops)']
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
