"""Cost of the position-table gradient (esme_hip_embed_positions_bwd) next to torch's two routes to the same sum, timed in the same run.

  python tools/embed_positions_bwd_bench.py [--reps 50] [--warmup 10] [--out profiles/embed_positions_bwd_bench.txt]

T = 50 000 packed rows, E = 1280, P = 4098 (the table of the released ESM-1b / ESM-1v files), three batches:
  * 13 x 3 846 rows: what tools/position_finetune.py and the reference's workflow train on (50 000-token batches of long proteins);
  * 100 x 500 rows;
  * 5 000 x 10 rows: the weak case -- ten table rows, each lane walks 5 000 sequences; correct, not meant to be fast.
HIP events around each call, the median of --reps calls after --warmup; outputs are allocated once, outside the timed calls.
Reported per batch:
  * esme_hip_embed_positions_bwd, and its bytes over time as a share of the ~6.3 TB/s a streaming kernel reaches
    (profiles/optim_bench.txt): dX read once, the table written once;
  * (a) torch.zeros(P, E, fp32).index_add_(0, pos + 2, dX.float()).bfloat16(): fp32 accumulation, but atomics (not bit-equal from run
    to run) and an fp32 copy of dX;
  * (b) torch's own F.embedding backward in bf16: what autograd runs for nn.Embedding;
  * the largest difference of each from a float64 sum, in units of the bf16 spacing of the result.
No ratio is a condition: the numbers are written down as measured.  Then the whole-step cost of training the table: one training step
of a two-layer model of ESM-1v's width (E = 1280, H = 20) on 100 x 500 rows, mark_trainable(positions='frozen') against
mark_trainable(positions=True)."""
import argparse
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'esm-efficient_amd')]
BATCHES = ((13, 3846), (100, 500), (5000, 10))


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
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--step-layers', type=int, default=2, help='layers of the ESM-1v-width model of the training-step leg (0: skip it)')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    from esme import _hip, _hip_embed_positions_bwd as HP, synthetic as syn
    dev, T, E, P, off = 'cuda:0', 50000, 1280, 4098, 2
    dx = torch.randn(T, E, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(dev)
    dp = torch.empty(P, E, dtype=torch.bfloat16, device=dev)
    acc = torch.zeros(P, E, dtype=torch.float32, device=dev)
    lines = [f'position-table gradient dP[p + 2] = sum over the sequences longer than p of their row p of dX; T = {T}, E = {E}, P = {P}, bf16; '
             f'median of {args.reps} calls after {args.warmup} warm-ups, HIP events',
             f'device {torch.cuda.get_device_name(0)}']
    for B, n in BATCHES:
        lengths = [n] * B
        rows = sum(lengths)
        cu = syn.cu_lens_of(lengths).to(dev)
        x = dx[:rows]
        idx = (_hip.seq_positions(cu, rows)[0].long() + off)
        ours = timed(lambda: HP.embed_positions_bwd(x, cu, P, off, n, d_pos=dp), args.warmup, args.reps)
        got = dp.clone()

        def route_a():
            return acc.zero_().index_add_(0, idx, x.float()).bfloat16()
        a = timed(route_a, args.warmup, args.reps)
        table = torch.zeros(P, E, dtype=torch.bfloat16, device=dev, requires_grad=True)
        y = torch.nn.functional.embedding(idx, table)

        def route_b():
            return torch.autograd.grad(y, table, x, retain_graph=True)[0]
        b = timed(route_b, args.warmup, args.reps)
        ref = torch.zeros(P, E, dtype=torch.float64, device=dev).index_add_(0, idx, x.double())
        spacing = torch.exp2(torch.floor(torch.log2(ref.abs().clamp(min=1e-30))) - 7)
        worst = lambda t: float(((t.double() - ref).abs() / spacing)[off:off + n].max())
        moved = rows * E * 2 + P * E * 2
        verdict = 'not slower than (a)' if ours[0] <= a[0] else f'SLOWER than (a) by {100 * (ours[0] / a[0] - 1):.0f} %'
        lines += [f'{B} x {n} rows: a fan-in of {B} on {n} table rows, {n * E // 8} work items that sum',
                  f'  esme_hip_embed_positions_bwd         {ours[0] * 1e3:9.1f} us (min {ours[1] * 1e3:.1f}, max {ours[2] * 1e3:.1f})   one launch, no workspace',
                  f'      moves {moved / 1e6:.1f} MB (dX once, the table written once): {moved / (ours[0] * 1e-3) / 1e12:.2f} TB/s = '
                  f'{100 * moved / (ours[0] * 1e-3) / 6.3e12:.0f} % of the ~6.3 TB/s a streaming kernel reaches',
                  f'      worst difference from the float64 sum: {worst(got):.2f} bf16 spacings; dead rows zero: {not bool(got[off + n:].any())}',
                  f'  (a) fp32 index_add_ + .bfloat16()    {a[0] * 1e3:9.1f} us (min {a[1] * 1e3:.1f}, max {a[2] * 1e3:.1f})   ours / (a) = {ours[0] / a[0]:.3f}  ({verdict})',
                  f'      worst difference from the float64 sum: {worst(route_a()):.2f} bf16 spacings; two runs bit-equal: {torch.equal(route_a(), route_a())}',
                  f'  (b) F.embedding backward in bf16     {b[0] * 1e3:9.1f} us (min {b[1] * 1e3:.1f}, max {b[2] * 1e3:.1f})   ours / (b) = {ours[0] / b[0]:.3f}',
                  f'      worst difference from the float64 sum: {worst(route_b()):.2f} bf16 spacings; two runs bit-equal: {torch.equal(route_b(), route_b())}']
    if args.step_layers > 0:
        import esme
        from esme import ESM
        L, H, n_seq, rows = args.step_layers, 20, 100, 500
        with tempfile.TemporaryDirectory() as td:
            model = ESM.from_pretrained(syn.write_checkpoint(os.path.join(td, 'm.safetensors'), 'esm1v_w650', L, E, H, seed=0), device=dev)
        model.train()
        lengths = [rows] * n_seq
        tokens, cu = syn.random_tokens(lengths, 4).to(dev), syn.cu_lens_of(lengths).to(dev)
        mask = torch.rand(tokens.numel(), generator=torch.Generator().manual_seed(2)).lt(0.15).to(dev)
        tokens_in = torch.where(mask, torch.full_like(tokens, model.alphabet.mask_idx), tokens)

        def step():
            model.zero_grad(set_to_none=True)
            logits = model.forward_trainable(tokens_in, (cu, rows))
            esme.cross_entropy(logits, tokens, mask, alphabet=model.alphabet).backward()
        w, r = 3, max(10, args.reps // 5)
        model.mark_trainable(positions='frozen').mark_lmhead(True)
        off_t = timed(step, w, r)
        model.mark_trainable(positions=True)
        on_t = timed(step, w, r)
        lines += [f'training step, {L} layers of ESM-1v width {E} (H = {H}), {n_seq} x {rows} rows, masked-token cross entropy, projections and LayerNorms trainable:',
                  f"  mark_trainable(positions='frozen')   {off_t[0]:8.3f} ms (min {off_t[1]:.3f}, max {off_t[2]:.3f})",
                  f'  mark_trainable(positions=True)       {on_t[0]:8.3f} ms (min {on_t[1]:.3f}, max {on_t[2]:.3f})   trained / frozen = {on_t[0] / off_t[0]:.4f}']
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
