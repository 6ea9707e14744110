"""Time the attention-pooling kernels against segment_mean on the same embeddings (HIP events, warm-up, repeats, spread).

  python tools/attn_pool_bench.py [--forward-ms 62.3] [--reps 50] [--out profiles/attn_pool_bench.txt]

Batches (E = 1280, H = 20, bf16 embeddings, the ESM2-650M width):
  uniform    T = 50 000 rows in 100 sequences of 500;
  proteome   tools/proteome_bench.py-style lengths (log-normal around 350, clipped to 30 .. 3 500) up to 50 000 rows;
  long       one 35 000-row sequence.
For each: attn_pool_fold, attn_pool (its two launches), fold + pool, the whole BinaryLearnedAggregation head, and segment_mean,
at n_cls = 1 and 4.  GB/s counts one read of x (T * E * 2 bytes).  The head's share is against --forward-ms, the ESM2-650M forward
of bench.py on a 50 000-token batch (measured in the same job by the caller)."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'esm-efficient_amd')]

from esme import _hip  # noqa: E402
from esme.pooling import BinaryLearnedAggregation, LearnedAggregation  # noqa: E402


def timed(fn, reps, warmup=5):
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
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return statistics.median(ts), ts[0], ts[-1]


def batches(T=50_000, seed=0):
    rng = np.random.default_rng(seed)
    lens, tot = [], 0
    while True:
        n = int(np.clip(round(rng.lognormal(math.log(350), 0.75)), 30, 3500))
        if tot + n > T:
            break
        lens.append(n)
        tot += n
    return {'uniform': [500] * (T // 500), 'proteome': lens, 'long': [35_000]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--forward-ms', type=float, default=None)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device (no CPU timing)'
    _hip.load()
    E, H = 1280, 20
    lines = [f'# attn_pool_bench: E={E} H={H} bf16 x, median (min..max) of {a.reps} reps after 5 warm-up, HIP events; '
             f'GB/s = one read of x over the median']
    rows = []
    for name, lens in batches().items():
        T = sum(lens)
        x = torch.randn(T, E, device='cuda').to(torch.bfloat16)
        cu = torch.zeros(len(lens) + 1, dtype=torch.int32)
        cu[1:] = torch.tensor(lens).cumsum(0)
        cu = cu.cuda()
        gb = T * E * 2 / 1e9
        for n_cls in (1, 4):
            head = (BinaryLearnedAggregation(H, E) if n_cls == 1 else LearnedAggregation(n_cls, H, E)).cuda()
            cls, wk = head.attn.cls, head.attn.k.weight
            U = _hip.attn_pool_fold(cls, wk, H)
            res = {
                'fold': timed(lambda: _hip.attn_pool_fold(cls, wk, H), a.reps),
                'pool': timed(lambda: _hip.attn_pool(x, cu, U, H, n_cls), a.reps),
                'fold+pool': timed(lambda: _hip.attn_pool(x, cu, _hip.attn_pool_fold(cls, wk, H), H, n_cls), a.reps),
                'head': timed(lambda: head(x, (cu, 0)), a.reps),
                'segment_mean': timed(lambda: _hip.segment_mean(x, cu), a.reps),
            }
            for k, (med, lo, hi) in res.items():
                bw = '' if k in ('fold', 'head') else f'  {gb / (med * 1e-6):7.0f} GB/s'
                lines.append(f'{name:9s} B={len(lens):4d} T={T:6d} n_cls={n_cls}  {k:13s} {med:9.1f} us ({lo:.1f}..{hi:.1f}){bw}')
            r = {'batch': name, 'B': len(lens), 'T': T, 'n_cls': n_cls, **{k: v[0] for k, v in res.items()},
                 'pool_GBps': gb / (res['pool'][0] * 1e-6), 'segment_mean_GBps': gb / (res['segment_mean'][0] * 1e-6)}
            r['pool_vs_segment_mean_bw'] = r['pool_GBps'] / r['segment_mean_GBps']
            if a.forward_ms:
                r['head_share_of_forward'] = res['head'][0] * 1e-3 / a.forward_ms
                lines.append(f'{"":9s} head = {100 * r["head_share_of_forward"]:.3f} % of a {a.forward_ms:.1f} ms ESM2-650M forward; '
                             f'pool reads x at {r["pool_vs_segment_mean_bw"]:.2f}x the rate of segment_mean')
            rows.append(r)
        del x
    lines.append(json.dumps(rows))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
