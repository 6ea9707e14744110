"""Cost of the attention-pooling backward kernel (esme_hip_attn_pool_bwd) next to the forward pooling kernel, timed in the same run.

  python tools/attn_pool_bwd_bench.py [--reps 20] [--warmup 5] [--out profiles/attn_pool_bwd_bench.txt]

ESM2-650M's width (E = 1280, H = 20) on 100 sequences of 500 rows, bf16, random x / U / dO, at n_cls = 1 and at n_cls = 4.  HIP events
around each call, the median of --reps calls after --warmup; workspaces and outputs are allocated once, outside the timed calls.
Reported per n_cls:
  * the backward with dx (a trainable backbone) and without (a frozen one: the common case);
  * the forward pooling kernel (esme_hip_attn_pool) on the same operands, and the two backward / forward ratios;
  * GFLOP/s over the flops the backward EXECUTES, in units of one T x J x E product (2 T J E flops): the score pass and the dU
    partials, plus the dX pass when dx is wanted (the forward runs one such product and T J d more).
Then the kernel's share of one training step: a two-layer model of the 650M width (E = 1280, H = 20) with rank-16 adapters on a batch
of 20 x 500 rows, model.forward_trainable(logits=False) + BinaryLearnedAggregation.forward_trainable + sum-reduced MSE + backward,
timed with HIP events in the same process; the pooling backward of that batch (with dx) is timed alone and divided by the step.
A full 33-layer model spends 16 times as long in the backbone, so the share there is that much smaller.
There is no pass mark: nobody had measured these numbers before; they are what a later performance change starts from."""
import argparse
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'esm-efficient_amd')]


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


def kernel_times(n_seq, rows, E, H, n_cls, warmup, reps, dev):
    from esme import _hip, _hip_attn_pool_bwd as HB
    T, J = n_seq * rows, n_cls * H
    g = torch.Generator().manual_seed(1)
    x = torch.randn(T, E, generator=g).to(torch.bfloat16).to(dev)
    U = (torch.randn(J, E, generator=g) * (1.4426950408889634 / E ** 0.5)).to(dev)
    d_out = torch.randn(n_seq, n_cls, E, generator=g).to(torch.bfloat16).to(dev)
    cu = (torch.arange(n_seq + 1, dtype=torch.int32) * rows).to(dev)
    ws = torch.empty(HB.workspace_bytes(n_seq, T, E, H, n_cls), dtype=torch.uint8, device=dev)
    dx = torch.zeros(T, E, dtype=torch.bfloat16, device=dev)
    fwd = timed(lambda: _hip.attn_pool(x, cu, U, H, n_cls), warmup, reps)
    bwd = timed(lambda: HB.attn_pool_bwd(x, cu, U, d_out, H, n_cls, need_dx=True, dx=dx, workspace=ws), warmup, reps)
    bwd0 = timed(lambda: HB.attn_pool_bwd(x, cu, U, d_out, H, n_cls, need_dx=False, workspace=ws), warmup, reps)
    return fwd, bwd, bwd0, 2.0 * T * J * E, ws.numel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--step-layers', type=int, default=2, help='layers of the 650M-width model of the training-step leg (0: skip it)')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    dev, E, H, n_seq, rows = 'cuda:0', 1280, 20, 100, 500
    lines = [f'attention-pooling backward, E = {E}, H = {H}, bf16, {n_seq} sequences x {rows} rows; median of {args.reps} calls after {args.warmup} warm-ups, HIP events',
             f'device {torch.cuda.get_device_name(0)}']
    for n_cls in (1, 4):
        fwd, bwd, bwd0, unit, nws = kernel_times(n_seq, rows, E, H, n_cls, args.warmup, args.reps, dev)
        lines += [f'n_cls = {n_cls} (J = {n_cls * H}), workspace {nws / 2 ** 20:.1f} MiB',
                  f'  backward with dx    {bwd[0]:8.3f} ms (min {bwd[1]:.3f}, max {bwd[2]:.3f})   {3 * unit / (bwd[0] * 1e-3) / 1e9:8.1f} GFLOP/s executed (3 T J E products)',
                  f'  backward without dx {bwd0[0]:8.3f} ms (min {bwd0[1]:.3f}, max {bwd0[2]:.3f})   {2 * unit / (bwd0[0] * 1e-3) / 1e9:8.1f} GFLOP/s executed (2 T J E products)',
                  f'  forward             {fwd[0]:8.3f} ms (min {fwd[1]:.3f}, max {fwd[2]:.3f})   {unit / (fwd[0] * 1e-3) / 1e9:8.1f} GFLOP/s executed (1 T J E product)',
                  f'  backward / forward = {bwd[0] / fwd[0]:.2f} with dx, {bwd0[0] / fwd[0]:.2f} without']
    if args.step_layers > 0:
        import torch.nn.functional as F
        from esme import ESM, synthetic as syn
        from esme.pooling import BinaryLearnedAggregation
        L, n_seq, rows = args.step_layers, 20, 500
        with tempfile.TemporaryDirectory() as td:
            model = ESM.from_pretrained(syn.write_checkpoint(os.path.join(td, 'm.safetensors'), 'esm2_w650', L, E, H, seed=0), device=dev)
        model.add_lora(rank=16, alpha=16)
        model.train()
        head = BinaryLearnedAggregation(H, E).to(dev).requires_grad_(True)
        with torch.no_grad():
            for p in head.parameters():
                p.normal_(0, p.shape[-1] ** -0.5)
        lengths = [rows] * n_seq
        tokens, cu = syn.random_tokens(lengths, 4).to(dev), syn.cu_lens_of(lengths).to(dev)
        labels = torch.randn(n_seq, device=dev)

        def step():
            model.zero_grad(set_to_none=True)
            head.zero_grad(set_to_none=True)
            rep = model.forward_trainable(tokens, (cu, rows), logits=False)
            F.mse_loss(head.forward_trainable(rep, (cu, rows)).float(), labels, reduction='sum').backward()
        st = timed(step, max(2, args.warmup // 2), max(5, args.reps // 2))
        _, bwd, _, _, _ = kernel_times(n_seq, rows, E, H, 1, args.warmup, args.reps, dev)
        lines += [f'training step, {L} layers of width {E} (H = {H}), rank-16 adapters, {n_seq} x {rows} rows, BinaryLearnedAggregation head, sum MSE:',
                  f'  forward_trainable + backward {st[0]:8.3f} ms (min {st[1]:.3f}, max {st[2]:.3f})',
                  f'  pooling backward with dx on that batch {bwd[0]:8.3f} ms = {100 * bwd[0] / st[0]:.2f} % of the step']
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
