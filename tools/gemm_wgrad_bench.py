"""Cost of the weight-gradient GEMM (esme_hip_gemm_wgrad) next to torch's own dy.t() @ x and to this project's forward GEMM, timed in
the same run.

  python tools/gemm_wgrad_bench.py [--reps 20] [--warmup 5] [--rows 50000] [--out profiles/gemm_wgrad_bench.txt]

M = 50 000 packed rows and the four projection shapes of ESM2-650M, (N, K) = (1280, 1280) q / k / v / out, (5120, 1280) FFN up,
(1280, 5120) FFN down, (3840, 1280) a packed QKV; bf16, random dy / x.  HIP events around each call, the median of --reps calls after
--warmup; workspaces and outputs are allocated once, outside the timed calls.  Reported per shape:
  * esme_hip_gemm_wgrad with db and without, bf16 outputs, its row chunks and workspace, and TFLOP/s over 2 M N K flops;
  * torch's dy.t() @ x on the same operands (the vendor BLAS; what F.linear's backward runs), and the ratio -- the aim is <= 1;
  * this project's forward GEMM _hip.gemm at the same (M, N, K): the same flops with the contraction along the rows' memory order.
Then one training step of a two-layer model of the 650M width (E = 1280, H = 20) on a batch of 20 x 500 rows, forward_trainable +
esme.cross_entropy + backward, frozen (LM head trainable only, so that a backward runs) against fully trainable (mark_trainable()).
There is no pass mark: nobody had measured these numbers before; they are what a later performance change starts from."""
import argparse
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'esm-efficient_amd')]
SHAPES = ((1280, 1280), (5120, 1280), (1280, 5120), (3840, 1280))


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


def shape_times(M, N, K, warmup, reps, dev):
    from esme import _hip, _hip_gemm_wgrad as HW
    g = torch.Generator().manual_seed(1)
    dy = torch.randn(M, N, generator=g).to(torch.bfloat16).to(dev)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16).to(dev)
    nws = HW.workspace_bytes(M, N, K)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
    dw, db = torch.empty(N, K, dtype=torch.bfloat16, device=dev), torch.empty(N, dtype=torch.bfloat16, device=dev)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    ours = timed(lambda: HW.gemm_wgrad(dy, x, dw=dw, db=db, workspace=ws), warmup, reps)
    ours0 = timed(lambda: HW.gemm_wgrad(dy, x, dw=dw, workspace=ws), warmup, reps)
    tor = timed(lambda: torch.matmul(dy.t(), x, out=dw), warmup, reps)
    fwd = timed(lambda: _hip.gemm(x, w, out=out), warmup, reps)
    return ours, ours0, tor, fwd, nws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rows', type=int, default=50000)
    ap.add_argument('--step-layers', type=int, default=2, help='layers of the 650M-width model of the training-step leg (0: skip it)')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    dev, M = 'cuda:0', args.rows
    lines = [f'weight-gradient GEMM dW = dY^T X (+ db), M = {M} rows, bf16; median of {args.reps} calls after {args.warmup} warm-ups, HIP events',
             f'device {torch.cuda.get_device_name(0)}']
    for N, K in SHAPES:
        ours, ours0, tor, fwd, nws = shape_times(M, N, K, args.warmup, args.reps, dev)
        tf = lambda ms: 2.0 * M * N * K / (ms * 1e-3) / 1e12
        chunks = nws // ((N * K + N) * 4) if nws else 1
        verdict = 'at or under torch' if ours[0] <= tor[0] else f'{100 * (ours[0] / tor[0] - 1):.0f} % over torch'
        lines += [f'(N, K) = ({N}, {K}): {chunks} row chunk(s), workspace {nws / 2 ** 20:.1f} MiB',
                  f'  esme_hip_gemm_wgrad with db {ours[0]:8.3f} ms (min {ours[1]:.3f}, max {ours[2]:.3f})   {tf(ours[0]):7.1f} TFLOP/s',
                  f'  esme_hip_gemm_wgrad, no db  {ours0[0]:8.3f} ms (min {ours0[1]:.3f}, max {ours0[2]:.3f})   {tf(ours0[0]):7.1f} TFLOP/s',
                  f'  torch dy.t() @ x            {tor[0]:8.3f} ms (min {tor[1]:.3f}, max {tor[2]:.3f})   {tf(tor[0]):7.1f} TFLOP/s   ours / torch = {ours[0] / tor[0]:.2f} ({verdict})',
                  f'  forward _hip.gemm (M, N, K) {fwd[0]:8.3f} ms (min {fwd[1]:.3f}, max {fwd[2]:.3f})   {tf(fwd[0]):7.1f} TFLOP/s   ours / forward = {ours[0] / fwd[0]:.2f}']
    if args.step_layers > 0:
        import esme
        from esme import ESM, synthetic as syn
        L, E, H, n_seq, rows = args.step_layers, 1280, 20, 20, 500
        with tempfile.TemporaryDirectory() as td:
            model = ESM.from_pretrained(syn.write_checkpoint(os.path.join(td, 'm.safetensors'), 'esm2_w650', L, E, H, seed=0), device=dev)
        model.train()
        lengths = [rows] * n_seq
        tokens, cu = syn.random_tokens(lengths, 4).to(dev), syn.cu_lens_of(lengths).to(dev)
        mask = torch.rand(tokens.numel(), generator=torch.Generator().manual_seed(2)).lt(0.3).to(dev)
        tokens_in = torch.where(mask, torch.full_like(tokens, model.alphabet.mask_idx), tokens)

        def step():
            model.zero_grad(set_to_none=True)
            esme.cross_entropy(model.forward_trainable(tokens_in, (cu, rows)), tokens, mask, alphabet=model.alphabet).backward()
        w, r = max(2, args.warmup // 2), max(5, args.reps // 2)
        model.mark_lmhead(True)
        frozen = timed(step, w, r)
        model.mark_trainable()
        full = timed(step, w, r)
        lines += [f'training step, {L} layers of width {E} (H = {H}), {n_seq} x {rows} rows, masked-token cross entropy, LM head trainable:',
                  f'  backbone frozen              {frozen[0]:8.3f} ms (min {frozen[1]:.3f}, max {frozen[2]:.3f})',
                  f'  backbone trainable           {full[0]:8.3f} ms (min {full[1]:.3f}, max {full[2]:.3f})   trainable / frozen = {full[0] / frozen[0]:.2f}']
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
