"""Cost of the transposing expansion of quantised weights (esme_hip_dequantize_*_t) and of one LoRA training step over a quantised base.

  python tools/qlora_bench.py [--reps 50] [--warmup 10] [--out profiles/qlora_bench.txt]

One process, medians.  The expansions take a few microseconds, less than the host needs to enqueue a call, so they are timed on the
device alone: --inner calls are captured into one hipGraph (a single chain, no branches) and HIP events go around a replay.  Per projection shape of ESM2-650M, (N, K) = (1280, 1280) q / k / v / out,
(5120, 1280) FFN up, (1280, 5120) FFN down, (3840, 1280) a packed QKV, in 4-bit and int8:
  * the transposed expansion into a preallocated (K, N) buffer, and the bytes it must move (0.5 N K + 2 N K for 4-bit, N K + 2 N K for
    int8; absmax / scales are left out) over its time;
  * the plain expansion of the same matrix (esme_hip_dequantize_*: the same bytes) and the ratio;
  * lin.dequantize().t().contiguous(): the plain expansion plus torch's transposing copy, the alternative the kernel replaces.
Then one forward_trainable + backward step of the two-layer ESM2-650M-width model of tools/gemm_wgrad_bench.py (20 x 500 rows, rank-16
adapters on q / v / out, masked-token cross entropy): the quantised base ('4bit', '8bit') against the bfloat16 base, re-measured in the
same process (HIP events around each step).  torch.cuda.max_memory_allocated over two steps is taken for each base in a child process
of its own that holds nothing but that model.  Loading a quantised model runs one fp32 torch matrix-vector product per LayerNorm-folded
matrix (c2 = W beta, esme.quantization.Q4Matrix), and the first such call makes torch allocate its BLAS workspace (128 MiB here) for
the life of the process; the bfloat16 model's step never makes one.  The bfloat16 base is therefore measured twice: as it is, and in a
process that made one fp32 matrix-vector product first, which is the like-for-like line.
There is no pass mark: nobody had measured these numbers before."""
import argparse
import gc
import os
import statistics
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'esm-efficient_amd'), os.path.join(ROOT, 'tools')]
from gemm_wgrad_bench import SHAPES, timed          # noqa: E402


def graph_timed(fn, warmup, reps, inner):
    """Median, min, max device time of one call in ms: `inner` calls captured into one graph, events around each of `reps` replays."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(inner):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return statistics.median(ts), min(ts), max(ts)


def shape_lines(N, K, warmup, reps, inner, dev):
    from esme import _hip, _hip_dequant_t as HT
    from esme.quantization import FP4_CODEBOOK
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16).to(dev)
    out, out_t = torch.empty(N, K, dtype=torch.bfloat16, device=dev), torch.empty(K, N, dtype=torch.bfloat16, device=dev)
    lines = []
    for bits in (4, 8):
        if bits == 4:
            codes, absmax = _hip.quantize_4bit(w, FP4_CODEBOOK)
            plain = lambda: _hip.dequantize_4bit(codes, absmax, FP4_CODEBOOK, out=out)
            trans = lambda: HT.dequantize_4bit_t(codes, absmax, FP4_CODEBOOK, out=out_t)
        else:
            codes, absmax = _hip.quantize_8bit(w)
            plain = lambda: _hip.dequantize_8bit(codes, absmax, out=out)
            trans = lambda: HT.dequantize_8bit_t(codes, absmax, out=out_t)
        assert torch.equal(trans(), plain().t())
        nbytes = (0.5 if bits == 4 else 1.0) * N * K + 2.0 * N * K
        t, p = graph_timed(trans, warmup, reps, inner), graph_timed(plain, warmup, reps, inner)
        c = graph_timed(lambda: plain().t().contiguous(), warmup, reps, inner)
        rate = lambda ms: nbytes / (ms * 1e-3) / 1e12
        lines += [f'(N, K) = ({N}, {K}) {bits}-bit: {nbytes / 2 ** 20:.1f} MiB to move',
                  f'  transposed expansion          {1e3 * t[0]:8.1f} us (min {1e3 * t[1]:.1f}, max {1e3 * t[2]:.1f})   {rate(t[0]):5.2f} TB/s',
                  f'  plain expansion               {1e3 * p[0]:8.1f} us (min {1e3 * p[1]:.1f}, max {1e3 * p[2]:.1f})   {rate(p[0]):5.2f} TB/s   transposed / plain = {t[0] / p[0]:.2f}',
                  f'  dequantize().t().contiguous() {1e3 * c[0]:8.1f} us (min {1e3 * c[1]:.1f}, max {1e3 * c[2]:.1f})                transposed / that = {t[0] / c[0]:.2f}']
    return lines


BASES = {'bfloat16': None, '4bit': '4bit', '8bit': '8bit'}
MEMORY_LEGS = (('bfloat16', False), ('bfloat16', True), ('4bit', False), ('8bit', False))        # (base, an fp32 torch matvec first)
L, E, H, N_SEQ, ROWS = 2, 1280, 20, 20, 500


def step_of(path, quant, dev):
    """(model, step): the model of the training-step leg on the base `quant` and one forward_trainable + backward on its batch."""
    import esme
    from esme import ESM, synthetic as syn
    lengths = [ROWS] * N_SEQ
    tokens, cu = syn.random_tokens(lengths, 4).to(dev), syn.cu_lens_of(lengths).to(dev)
    mask = torch.rand(tokens.numel(), generator=torch.Generator().manual_seed(2)).lt(0.3).to(dev)
    model = ESM.from_pretrained(path, quantization=quant, device=dev).add_lora(rank=16, quantized_base=True).train()
    tokens_in = torch.where(mask, torch.full_like(tokens, model.alphabet.mask_idx), tokens)

    def step():
        model.zero_grad(set_to_none=True)
        esme.cross_entropy(model.forward_trainable(tokens_in, (cu, ROWS)), tokens, mask, alphabet=model.alphabet).backward()
    return model, step


def memory_leg(path, base, blas_first, dev):
    """In a process of its own: prints max_memory_allocated over two steps on the base `base`."""
    if blas_first:
        torch.mv(torch.ones(64, 64, device=dev), torch.ones(64, device=dev))
    model, step = step_of(path, BASES[base], dev)
    step()
    step()
    torch.cuda.synchronize()
    print(f'PEAK {torch.cuda.max_memory_allocated()}')


def step_lines(warmup, reps, dev):
    from esme import synthetic as syn
    lines = [f'training step, {L} layers of width {E} (H = {H}), {N_SEQ} x {ROWS} rows, rank-16 adapters on q / v / out, masked-token cross entropy:']
    base = None
    with tempfile.TemporaryDirectory() as td:
        path = syn.write_checkpoint(os.path.join(td, 'm.safetensors'), 'esm2_w650', L, E, H, seed=0)
        times = {}
        for name, quant in BASES.items():
            model, step = step_of(path, quant, dev)
            times[name] = timed(step, warmup, reps)
            del model, step
            gc.collect()
            torch.cuda.empty_cache()
        for name, t in times.items():
            lines.append(f'  {name:9s} base  {t[0]:8.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})   / bfloat16 = {t[0] / times["bfloat16"][0]:.2f}')
        lines.append('max_memory_allocated over two steps, each in a process of its own:')
        for name, blas_first in MEMORY_LEGS:                  # one child at a time, after this process's own timings
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--memory-of', name, '--checkpoint', path] +
                                 (['--blas-first'] if blas_first else []), check=True, capture_output=True, text=True, timeout=300).stdout
            peak = int(next(ln for ln in out.splitlines() if ln.startswith('PEAK ')).split()[1])
            if blas_first:
                base = peak
            lines.append(f'  {name:9s} base{", after one fp32 torch matvec" if blas_first else "":30s} {peak / 2 ** 20:8.1f} MiB' +
                         (f'   ({(peak - base) / 2 ** 20:+.1f} MiB against bfloat16 with the workspace)' if base and not blas_first else ''))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--inner', type=int, default=20, help='calls per captured graph')
    ap.add_argument('--out', default='')
    ap.add_argument('--memory-of', default='', help='(internal) run the memory leg of one base on --checkpoint and print its peak')
    ap.add_argument('--checkpoint', default='')
    ap.add_argument('--blas-first', action='store_true', help='(internal) the memory leg makes one fp32 torch matvec first')
    args = ap.parse_args()
    dev = 'cuda:0'
    if args.memory_of:
        return memory_leg(args.checkpoint, args.memory_of, args.blas_first, dev)
    lines = [f'transposing expansion of quantised weights (esme_hip_dequantize_*_t); median of {args.reps} replays of a graph of {args.inner} calls, HIP events around a replay',
             f'device {torch.cuda.get_device_name(0)}']
    for N, K in SHAPES:
        lines += shape_lines(N, K, args.warmup, args.reps, args.inner, dev)
    lines += step_lines(max(2, args.warmup // 2), max(5, args.reps // 5), dev)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
