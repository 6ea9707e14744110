"""Cost of the LoRA adapters on the module path (HIP events, warm-up, repeats, spread).

  python tools/lora_bench.py [--tree PATH] [--adapters 0|1|2] [--targets qvo|all] [--reps 10] [--trace] [--tag NAME]

ESM2-650M geometry (33 layers, E = 1 280, H = 20) with synthetic weights, 50 000 residues in 100 sequences of 500, precision 'fast',
the module-by-module forward (`c_forward = False`; a model with adapters always takes it).  One process measures ONE configuration
of ONE source tree and prints one JSON line; a job alternates processes to compare
  * adapters off in this tree against the parent commit's tree (`--tree`: a checkout with its library built; a tree without
    esme.lora can only run --adapters 0), at least 3 pairs, pass mark "inside the spread of the parent against itself";
  * --adapters 1 / 2 (rank 16 on q / v / out, one or two adapters, lora_B filled) against --adapters 0;
  * --targets all: the adapters on all six targets (query, key, value, output, ffn_up, ffn_down -- every linear layer of the block, the
    QLoRA recipe) instead of q / v / out.
`--trace`: per-kernel HIP-event times of one forward through esme._hip.TRACE (esme_hip_lora_down, the extended GEMMs), plus
esme_hip_segment_mean on the same residual stream as the yardstick for a kernel that reads x once (GB/s = T * K * 2 bytes / time with
K the width of what the launch reads: E, or the FFN width F for the down-projection's adapter).
Run `rocprofv3 --kernel-trace --stats -- python tools/lora_bench.py --adapters 1 --reps 3` in a run of its own for the profiler's view."""
import argparse
import json
import os
import statistics
import sys

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--adapters', type=int, default=0)
    ap.add_argument('--targets', choices=('qvo', 'all'), default='qvo')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--tag', default='')
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path[:0] = [tree, os.path.join(tree, 'esm-efficient_amd')]
    import tempfile
    from esme import ESM, _hip, synthetic as syn
    dev = 'cuda:0'
    with tempfile.TemporaryDirectory() as td:
        model = ESM.from_pretrained(syn.write_checkpoint(os.path.join(td, 'm.safetensors'), 'esm2_650m'), device=dev)
    model.c_forward = False
    if args.adapters:
        names = ['a', 'b'][:args.adapters]
        layers = ('query', 'value', 'output') if args.targets == 'qvo' else ('query', 'key', 'value', 'output', 'ffn_up', 'ffn_down')
        model.add_lora(rank=16, alpha=16, layers=layers, adapter_names=names)
        gen = torch.Generator().manual_seed(1)
        with torch.no_grad():
            for k, p in sorted(model.named_parameters()):
                if '.lora_B.' in k:
                    p.copy_((torch.randn(p.shape, generator=gen) * 0.02).to(p.dtype))
    tokens, cu, max_len, _ = syn.uniform_batch(50000, 500, seed=0)
    tokens, cu = tokens.to(dev), cu.to(dev)
    run = lambda: model(tokens, (cu, max_len))
    with torch.no_grad():
        for _ in range(args.warmup):
            run()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        out = {'tag': args.tag, 'tree': tree, 'adapters': args.adapters, 'targets': args.targets if args.adapters else None, 'reps': args.reps, 'ms_median': round(statistics.median(ts), 3),
               'ms_min': round(min(ts), 3), 'ms_max': round(max(ts), 3)}
        if args.trace:
            T, E = tokens.numel(), model.embed_dim
            _hip.TRACE = []
            run()
            x = torch.randn(T, E, device=dev).bfloat16()
            for _ in range(5):
                with _hip._Traced('segment_mean', (T, E)):
                    _hip.segment_mean(x, cu)
            torch.cuda.synchronize()
            trace, _hip.TRACE = _hip.TRACE, None
            per = {}
            for op, meta, s, e in trace:
                key = f'{op} {meta}'
                per.setdefault(key, []).append(s.elapsed_time(e) * 1e3)
            rows = {}
            for key, v in per.items():
                if key.startswith(('lora_down', 'segment_mean', 'gemm')):
                    rows[key] = {'n': len(v), 'us_median': round(statistics.median(v), 1), 'us_min': round(min(v), 1), 'us_max': round(max(v), 1)}
            for op, meta, _, _ in trace:                              # (read rate: the width of what the launch reads -- lora_down's meta is (T, X, K, ln))
                if op in ('lora_down', 'segment_mean'):
                    row = rows[f'{op} {meta}']
                    row['GBps_x_read'] = round(T * (meta[2] if op == 'lora_down' else E) * 2 / (row['us_median'] * 1e-6) / 1e9, 1)
            out['kernels'] = rows
    print(json.dumps(out))


if __name__ == '__main__':
    main()
