"""Cost of the mean-pool backward (esme_hip_segment_mean_bwd) next to the torch ops it replaced, and of layer taps in a training step.

  python tools/segment_mean_bwd_bench.py [--reps 50] [--warmup 10] [--out profiles/segment_mean_bwd_bench.txt]
                                         [--step-out profiles/taps_train_bench.txt]

Kernel leg.  T = 50 000 packed rows, E = 1280, B = 100 sequences of proteome-like lengths, bf16.  The two routes are timed in the same
run, alternating, with HIP events around each call (median of --reps after --warmup; d_x is allocated outside the timed calls for the
kernel, inside for the torch route, as autograd ran it):
  * esme_hip_segment_mean_bwd, and the bytes it must move (d_x written once, d_y read once) over its time as a share of the
    ~6.3 TB/s a streaming kernel reaches (profiles/optim_bench.txt);
  * the torch backward of esme.autograd.SegmentMean as it was: divide, zeros, repeat_interleave with tensor repeats, a host read of
    cu_lens[0], an indexed copy -- the same bits, checked here;
  * what the two host synchronisations of that route cost a training step: the host time until the backward call RETURNS when the
    stream still holds queued work (--queued-ms of GEMMs).  A route without a synchronisation returns after its enqueue; a route
    with one returns only when everything queued before it has run, so the host cannot run ahead and the device idles while the
    host prepares the next launches.
Expectation to confirm or refute: the kernel is not slower than the torch route.

Step leg (--step-out).  One forward_trainable + backward step of a two-layer model of the 650M width (E = 1280, H = 20; the model of
profiles/gemm_wgrad_bench.txt) on 20 x 500 rows with every projection and LayerNorm trainable and a BinaryLearnedAggregation head,
summed-MSE loss: with layers=[0] (head width 2 E) against no taps (head width E).  The difference is what the taps cost."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'esm-efficient_amd')]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternating(fns, warmup, reps):
    """Median, min, max of the event time of every fn, the fns taking turns."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ts[i].append(event_ms(fn))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def torch_backward(dy, cu_lens, rows):
    """esme.autograd.SegmentMean.backward before the kernel existed."""
    lens = (cu_lens[1:] - cu_lens[:-1]).to(torch.long)
    g = (dy.float() / lens.clamp(min=1).view(-1, 1)).to(dy.dtype)
    dx = torch.zeros(rows, dy.shape[1], dtype=dy.dtype, device=dy.device)
    seg = torch.repeat_interleave(torch.arange(lens.numel(), device=dy.device), lens)
    start = int(cu_lens[0])
    dx[start:start + seg.numel()] = g[seg]
    return dx


def lengths_summing_to(T, B, seed=0):
    g = torch.Generator().manual_seed(seed)
    w = torch.exp(0.75 * torch.randn(B, generator=g, dtype=torch.float64))       # log-normal, like a proteome's lengths
    lens = torch.clamp((w / w.sum() * T).floor().long(), min=1)
    lens[-1] += T - int(lens.sum())
    assert int(lens.sum()) == T and int(lens.min()) > 0
    return lens.tolist()


def host_return_ms(fn, queue, reps):
    """Median host time until fn() returns when `queue()` has just filled the stream."""
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        queue()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
    return statistics.median(ts)


def kernel_leg(args, dev):
    from esme import _hip_segment_mean_bwd as HS, synthetic as syn
    T, E, B = args.rows, 1280, args.sequences
    lens = lengths_summing_to(T, B)
    cu = syn.cu_lens_of(lens).to(dev)
    dy = torch.randn(B, E, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(dev)
    dx = torch.empty(T, E, dtype=torch.bfloat16, device=dev)
    ours_fn = lambda: HS.segment_mean_bwd(dy, cu, T, d_x=dx)
    torch_fn = lambda: torch_backward(dy, cu, T)
    same = torch.equal(ours_fn(), torch_fn())
    ours, ref = alternating([ours_fn, torch_fn], args.warmup, args.reps)
    a = torch.randn(8192, 8192, device=dev, dtype=torch.bfloat16)
    one = statistics.median(event_ms(lambda: a @ a) for _ in range(5))
    n_q = max(1, round(args.queued_ms / one))
    queue = lambda: [a @ a for _ in range(n_q)]
    ret_ours, ret_ref = host_return_ms(ours_fn, queue, 10), host_return_ms(torch_fn, queue, 10)
    moved = T * E * 2 + B * E * 2
    verdict = 'not slower than the torch route' if ours[0] <= ref[0] else f'SLOWER than the torch route by {100 * (ours[0] / ref[0] - 1):.0f} %'
    return [f'mean-pool backward dX[t] = dY[s(t)] / len_s; T = {T}, E = {E}, B = {B} (lengths {min(lens)} .. {max(lens)}), bf16; median of {args.reps} '
            f'calls after {args.warmup} warm-ups, HIP events, the two routes alternating',
            f'device {torch.cuda.get_device_name(0)}',
            f'  esme_hip_segment_mean_bwd            {ours[0] * 1e3:9.1f} us (min {ours[1] * 1e3:.1f}, max {ours[2] * 1e3:.1f})   {-(-T // HS.ROWS)} workgroups of {HS.ROWS} rows, one launch',
            f'      moves {moved / 1e6:.1f} MB (d_x written once, d_y read once): {moved / (ours[0] * 1e-3) / 1e12:.2f} TB/s = '
            f'{100 * moved / (ours[0] * 1e-3) / 6.3e12:.0f} % of the ~6.3 TB/s a streaming kernel reaches',
            f'  torch ops (the backward as it was)   {ref[0] * 1e3:9.1f} us (min {ref[1] * 1e3:.1f}, max {ref[2] * 1e3:.1f})   ours / torch = {ours[0] / ref[0]:.3f}  ({verdict})',
            f'      the same bits: {same}',
            f'host time until the backward call returns behind {n_q} queued 8192^3 GEMMs ({n_q * one:.1f} ms of device work), median of 10:',
            f'  esme_hip_segment_mean_bwd            {ret_ours:9.3f} ms   (the enqueue: the host runs ahead of the device)',
            f'  torch ops                            {ret_ref:9.3f} ms   (two synchronisations: the host waits for the queue to drain, twice over nothing new)']


def step_leg(args, dev):
    import torch.nn.functional as F
    from esme import ESM, synthetic as syn
    from esme.pooling import BinaryLearnedAggregation
    from esme.trainer import RegressionModel
    L, E, H, n_seq, rows = args.step_layers, 1280, 20, 20, 500
    with tempfile.TemporaryDirectory() as td:
        model = ESM.from_pretrained(syn.write_checkpoint(os.path.join(td, 'm.safetensors'), 'esm2_w650', L, E, H, seed=0), device=dev)
    model.mark_trainable().train()
    lengths = [rows] * n_seq
    tokens, cu = syn.random_tokens(lengths, 4).to(dev), syn.cu_lens_of(lengths).to(dev)
    label = torch.rand(n_seq, generator=torch.Generator().manual_seed(3)).to(dev)
    nets = []
    for layers in (None, [0]):
        torch.manual_seed(0)
        head = BinaryLearnedAggregation(H, E * (1 + len(layers or ()))).to(dev).requires_grad_(True)
        nets.append(RegressionModel(model, head, layers=layers).train())

    def step(net):
        net.zero_grad(set_to_none=True)
        y = net.forward_trainable(tokens, (cu, rows))
        F.mse_loss(y.float(), label, reduction='sum').backward()
    plain, taps = alternating([lambda: step(nets[0]), lambda: step(nets[1])], 3, max(10, args.reps // 2))
    return [f'training step, {L} layers of width {E} (H = {H}), {n_seq} x {rows} rows, every projection and LayerNorm trainable, BinaryLearnedAggregation head, '
            f'summed MSE; forward_trainable + backward, median of {max(10, args.reps // 2)} steps after 3 warm-ups, HIP events, the two alternating',
            f'device {torch.cuda.get_device_name(0)}',
            f'  no taps (head width {E})                 {plain[0]:8.3f} ms (min {plain[1]:.3f}, max {plain[2]:.3f})',
            f'  layers=[0] (head width {2 * E})           {taps[0]:8.3f} ms (min {taps[1]:.3f}, max {taps[2]:.3f})   with / without = {taps[0] / plain[0]:.4f}',
            f'  the taps cost {taps[0] - plain[0]:+.3f} ms per step: the concatenation, a head of twice the width, and the sum of two gradients at the tapped layer']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rows', type=int, default=50000)
    ap.add_argument('--sequences', type=int, default=100)
    ap.add_argument('--queued-ms', type=float, default=20.0, help='device work queued ahead of the backward in the host-return leg')
    ap.add_argument('--step-layers', type=int, default=2, help='layers of the 650M-width model of the training-step leg (0: skip it)')
    ap.add_argument('--out', default='')
    ap.add_argument('--step-out', default='')
    args = ap.parse_args()
    dev = 'cuda:0'
    for lines, path in ((kernel_leg(args, dev), args.out), (step_leg(args, dev) if args.step_layers > 0 else [], args.step_out)):
        text = '\n'.join(lines)
        print(text)
        if path and lines:
            with open(path, 'w') as fh:
                fh.write(text + '\n')


if __name__ == '__main__':
    main()
