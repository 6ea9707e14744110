"""Cost of the fused linear + cross-entropy kernel (esme_hip_linear_xent_fwd / _bwd) next to the torch route it replaces, timed in
the same run on the same tensors.

  python tools/linear_xent_bench.py [--reps 30] [--warmup 5] [--rows 50000] [--out profiles/linear_xent_bench.txt]

T = 50 000 packed rows, E = 1280, C = 3 (a three-state per-residue task) and C = 33 (the vocabulary projection of the masked-LM head),
bf16, about half the rows labelled.  HIP events around forward + backward (dX, dW and db), the median of --reps after --warmup.
Reported per C:
  * the kernel route: esme.autograd.LinearCrossEntropy forward and backward, and the forward and the backward on their own;
  * the torch route: F.linear -> boolean row selection (logits[mask]: a nonzero) -> F.cross_entropy, forward and backward;
  * the share of the ~6.3 TB/s a streaming kernel reaches (profiles/optim_bench.txt), counting what the issue counts: one read of x per
    pass (forward, backward) plus one write of dX;
  * the host-return time of each route's forward + backward behind 20 ms of queued work: how long the host is held before it can go
    on queueing the optimiser step (the torch route waits for the queue to drain at its nonzero)."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

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


def host_return(fn, filler, reps=5):
    """Median host time of fn() in ms when about 20 ms of work is queued in front of it."""
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        filler()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rows', type=int, default=50000)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    from esme import _hip_linear_xent as HL
    from esme.autograd import LinearCrossEntropy
    dev, T, E = 'cuda:0', args.rows, 1280
    g = torch.Generator().manual_seed(0)
    x = torch.randn(T, E, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    a = torch.randn(4096, 4096, device=dev, dtype=torch.bfloat16)
    one = timed(lambda: a @ a, 3, 10)[0]
    n_fill = max(1, round(20.0 / one))

    def filler():
        for _ in range(n_fill):
            a @ a
    lines = [f'linear + cross-entropy over packed rows; T = {T}, E = {E}, bf16, about half the rows labelled; median of {args.reps} calls after '
             f'{args.warmup} warm-ups, HIP events', f'device {torch.cuda.get_device_name(0)}',
             f'queued work for the host-return time: {n_fill} x (4096^3 bf16 matmul of {one:.2f} ms) = {n_fill * one:.1f} ms']
    for C in (3, 33):
        w = (torch.randn(C, E, generator=g) / E ** 0.5).to(torch.bfloat16).to(dev).requires_grad_(True)
        b = torch.zeros(C, dtype=torch.bfloat16, device=dev, requires_grad=True)
        y = torch.randint(0, C, (T,), generator=g)
        y = torch.where(torch.rand(T, generator=g) < 0.5, torch.full_like(y, -100), y).to(dev)
        mask = y != -100

        def ours():
            x.grad = w.grad = b.grad = None
            LinearCrossEntropy.apply(x, w, b, y, -100, None, True).backward()

        def theirs():
            x.grad = w.grad = b.grad = None
            F.cross_entropy(F.linear(x, w, b)[mask], y[mask]).backward()
        xd, wd, bd = x.detach(), w.detach(), b.detach()
        one_grad = torch.ones(1, dtype=torch.float32, device=dev)
        wsf = torch.empty(HL.fwd_workspace_bytes(T), dtype=torch.uint8, device=dev)
        wsb = torch.empty(HL.bwd_workspace_bytes(T, E, C), dtype=torch.uint8, device=dev)
        dx = torch.empty(T, E, dtype=torch.bfloat16, device=dev)
        sums, _, lse = HL.linear_xent_fwd(xd, wd, bd, y, workspace=wsf)
        fwd = timed(lambda: HL.linear_xent_fwd(xd, wd, bd, y, workspace=wsf), args.warmup, args.reps)
        bwd = timed(lambda: HL.linear_xent_bwd(xd, wd, bd, y, lse, sums, one_grad, d_x=dx, workspace=wsb), args.warmup, args.reps)
        bwd_dx = timed(lambda: HL.linear_xent_bwd(xd, wd, bd, y, lse, sums, one_grad, want_dw=False, d_x=dx, workspace=wsb), args.warmup, args.reps)
        o, t = timed(ours, args.warmup, args.reps), timed(theirs, args.warmup, args.reps)
        ours()
        go = [x.grad.clone(), w.grad.clone()]
        l_o = float(LinearCrossEntropy.apply(x, w, b, y, -100, None, True).detach())
        theirs()
        l_t = float(F.cross_entropy(F.linear(x, w, b)[mask], y[mask]).detach())
        moved = 3 * T * E * 2
        h_o, h_t = host_return(ours, filler), host_return(theirs, filler)
        verdict = 'faster' if o[0] <= t[0] else f'SLOWER by {100 * (o[0] / t[0] - 1):.0f} %'
        lines += [f'C = {C}:',
                  f'  kernel route, forward + backward   {o[0] * 1e3:9.1f} us (min {o[1] * 1e3:.1f}, max {o[2] * 1e3:.1f})',
                  f'      esme_hip_linear_xent_fwd alone  {fwd[0] * 1e3:9.1f} us;  _bwd alone (dX, dW, db) {bwd[0] * 1e3:9.1f} us;  _bwd with dX only {bwd_dx[0] * 1e3:9.1f} us',
                  f'      x read once per pass and dX written once = {moved / 1e6:.0f} MB: {moved / ((fwd[0] + bwd[0]) * 1e-3) / 1e12:.2f} TB/s over the two '
                  f'calls = {100 * moved / ((fwd[0] + bwd[0]) * 1e-3) / 6.3e12:.0f} % of the ~6.3 TB/s a streaming kernel reaches '
                  f'(the backward reads x a second time for dW, which this count leaves out)',
                  f'      workspace: forward {wsf.numel() / 2 ** 10:.1f} KiB, backward {wsb.numel() / 2 ** 20:.1f} MiB',
                  f'  torch route, forward + backward    {t[0] * 1e3:9.1f} us (min {t[1] * 1e3:.1f}, max {t[2] * 1e3:.1f})   kernel / torch = {o[0] / t[0]:.3f}  ({verdict})',
                  f'  loss: kernel {l_o:.6f}, torch {l_t:.6f};  largest |dX| difference {float((go[0].float() - x.grad.float()).abs().max()):.3e}, '
                  f'|dW| difference {float((go[1].float() - w.grad.float()).abs().max()):.3e} (of max |dW| {float(w.grad.float().abs().max()):.3e})',
                  f'  host returns after forward + backward behind the queued work: kernel route {h_o:.3f} ms, torch route {h_t:.3f} ms']
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
