"""Cost of esme.optim.AdamW's fused step next to torch doing the same work, alternated in one process.

  python tools/optim_bench.py [--steps 20] [--warmup 5] [--layers 33] [--out profiles/optim_bench.txt]

No checkpoint is needed: the parameter list has the shapes of ESM2-650M after mark_trainable() -- per layer four (1280, 1280), one
(5120, 1280), one (1280, 5120), their biases and two LayerNorms, plus the final LayerNorm -- with random bf16 values and gradients; a
second list is LoRA-only, rank 16 on q / k / v / out.  Per list, after --warmup steps of each, --steps rounds of
  (A) esme.optim.AdamW(max_grad_norm=1.0).step(): one table upload, the norm's two launches, the fused step;
  (B) torch on fp32 masters: a foreach copy of the bf16 gradients to fp32, clip_grad_norm_, torch.optim.AdamW (fused=True where the
      build accepts it, foreach=True otherwise), a foreach copy of the masters into the bf16 parameters
alternate, each between two device events (the time from the step's first launch reaching the device to its last one finishing, host
gaps included), with the host time of the call next to it.  Reported: median, min and max per step; the bytes the algorithm needs per
parameter (a bf16 parameter with a bf16 gradient: 14 read and 14 written by the step, 2 more read by the norm pass: 30) and A's achieved
bytes/s against the ~6.3 TB/s a streaming kernel reaches on this part.  The acceptance condition is A <= B."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'esm-efficient_amd')]
HBM_ACHIEVABLE = 6.3e12


def full_shapes(layers, E=1280, F=5120):
    per = [(E, E), (E,)] * 4 + [(F, E), (F,), (E, F), (E,)] + [(E,), (E,)] * 2
    return per * layers + [(E,), (E,)]


def lora_shapes(layers, E=1280, rank=16):
    return [(rank, E), (E, rank)] * 4 * layers


def make(shapes, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    params = [torch.nn.Parameter((torch.randn(s, generator=g, device=dev) * 0.05).to(torch.bfloat16)) for s in shapes]
    grads = [(5e-4 + 1e-3 * torch.randn(s, generator=g, device=dev)).to(torch.bfloat16) for s in shapes]
    return params, grads


def bench(name, shapes, args, dev):
    import esme
    params_a, grads = make(shapes, dev, 0)
    params_b = [torch.nn.Parameter(p.detach().clone()) for p in params_a]
    n = sum(p.numel() for p in params_a)
    opt_a = esme.optim.AdamW(params_a, lr=1e-5, max_grad_norm=1.0)
    masters = [torch.nn.Parameter(p.detach().float()) for p in params_b]
    g32 = [torch.empty_like(m) for m in masters]
    for m, g in zip(masters, g32):
        m.grad = g
    try:
        opt_b, how = torch.optim.AdamW(masters, lr=1e-5, fused=True), 'fused=True'
    except (RuntimeError, ValueError):
        opt_b, how = torch.optim.AdamW(masters, lr=1e-5, foreach=True), 'foreach=True'
    raw_b = [p.detach() for p in params_b]
    raw_m = [m.detach() for m in masters]

    def step_a():
        for p, g in zip(params_a, grads):
            p.grad = g
        opt_a.step()

    def step_b():
        torch._foreach_copy_(g32, grads)
        torch.nn.utils.clip_grad_norm_(masters, 1.0, foreach=True)
        opt_b.step()
        torch._foreach_copy_(raw_b, raw_m)

    for _ in range(args.warmup):
        step_a()
        step_b()
    torch.cuda.synchronize()
    dev_ms, host_ms = {'A': [], 'B': []}, {'A': [], 'B': []}
    for _ in range(args.steps):
        for label, fn in (('A', step_a), ('B', step_b)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            host_ms[label].append(1e3 * (time.perf_counter() - t0))
            b.synchronize()
            dev_ms[label].append(a.elapsed_time(b))
    med = {k: statistics.median(v) for k, v in dev_ms.items()}
    rate = 30.0 * n / (med['A'] * 1e-3)
    verdict = 'A no slower than B' if med['A'] <= med['B'] else f'A is {100 * (med["A"] / med["B"] - 1):.0f} % SLOWER than B'
    lines = [f'{name}: {len(shapes)} tensors, {n / 1e6:.1f} M parameters (bf16 parameters and gradients), {args.steps} alternating steps after {args.warmup} warm-ups']
    for label, what in (('A', 'esme.optim.AdamW(max_grad_norm=1.0)'), ('B', f'torch: fp32 gradients, clip_grad_norm_, AdamW({how}) on fp32 masters, copy to bf16')):
        d, h = dev_ms[label], host_ms[label]
        lines.append(f'  ({label}) {what}\n      {statistics.median(d):8.3f} ms per step (min {min(d):.3f}, max {max(d):.3f}); host time of the call {statistics.median(h):.3f} ms')
    lines.append(f'  A / B = {med["A"] / med["B"]:.2f}  ({verdict})')
    lines.append(f'  A moves 30 B per parameter (14 read + 14 written by the step, 2 read by the norm pass; 28 without clipping): {30.0 * n / 1e9:.2f} GB per step, '
                 f'{rate / 1e12:.2f} TB/s = {100 * rate / HBM_ACHIEVABLE:.0f} % of the ~6.3 TB/s a streaming kernel reaches')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--layers', type=int, default=33)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('optim_bench.py measures on a HIP device; none is available')
    dev = 'cuda:0'
    lines = ['fused AdamW with fp32 master weights (esme_hip_optim_*) against torch on fp32 masters; device events around each step, alternating',
             f'device {torch.cuda.get_device_name(0)}']
    lines += bench(f'ESM2-650M after mark_trainable() ({args.layers} layers)', full_shapes(args.layers), args, dev)
    lines += bench(f'LoRA only, rank 16 on q / k / v / out ({args.layers} layers)', lora_shapes(args.layers), args, dev)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
