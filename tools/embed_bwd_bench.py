"""Cost of the token-embedding gradient (esme_hip_embed_bwd) next to torch's two routes to the same sum, timed in the same run.

  python tools/embed_bwd_bench.py [--reps 50] [--warmup 10] [--rows 50000] [--out profiles/embed_bwd_bench.txt]

T = 50 000 packed rows, E = 1280, V = 33 (ESM2-650M's table); the ids are proteins of about 350 residues drawn with the amino-acid
frequencies of a proteome (leucine about 10 %, tryptophan about 1 %), `<cls>` and `<eos>` once per protein, and 12 % of the residues
replaced by `<mask>` (what mask_tokens leaves at freq 0.15, alter 0.1), whose rows the kernel skips as the forward zeroes them.  HIP
events around each call, the median of --reps calls after --warmup; outputs and the workspace are allocated once, outside the timed
calls.  Reported:
  * esme_hip_embed_bwd, and its bytes over time as a share of the ~6.3 TB/s a streaming kernel reaches (profiles/optim_bench.txt):
    dX read once, the chunks' fp32 partials written and read once;
  * (a) torch.zeros(V, E, fp32).index_add_(0, tok, dX.float()).bfloat16(): fp32 accumulation, but atomics (not bit-equal from run to
    run) and an fp32 copy of dX;
  * (b) torch's own F.embedding backward in bf16: what autograd runs for nn.Embedding;
  * the largest difference of each from a float64 sum, in units of the bf16 spacing of the result.
The condition of the kernel's pull request: it is not slower than route (a) at this shape.  Then the whole-step cost of training the
table: one training step of ESM2-650M's geometry (33 layers, E = 1280, H = 20, checkpoint_layers=True) on 20 x 500 rows,
mark_trainable() against mark_trainable(embedding=True)."""
import argparse
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'esm-efficient_amd')]
# ids 4 .. 23 = L A G V S E R T I D P K Q N F Y M H W C, per cent of the residues of a proteome
FREQ = (9.9, 8.3, 7.1, 6.9, 6.6, 6.8, 5.5, 5.3, 5.9, 5.5, 4.7, 5.8, 3.9, 4.1, 3.9, 2.9, 2.4, 2.3, 1.1, 1.4)


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


def proteome_tokens(T, seed=0, length=350, mask_share=0.12):
    g = torch.Generator().manual_seed(seed)
    tok = 4 + torch.multinomial(torch.tensor(FREQ, dtype=torch.float64), T, replacement=True, generator=g)
    tok = torch.where(torch.rand(T, generator=g) < mask_share, torch.tensor(32), tok)
    tok[::length] = 0
    tok[length - 1::length] = 2
    tok[T - 1] = 2
    return tok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rows', type=int, default=50000)
    ap.add_argument('--step-layers', type=int, default=33, help='layers of the 650M-width model of the training-step leg (0: skip it)')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    from esme import _hip_embed_bwd as HE
    dev, T, E, V = 'cuda:0', args.rows, 1280, 33
    tok = proteome_tokens(T).to(dev)
    dx = torch.randn(T, E, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(dev)
    counts = torch.bincount(tok, minlength=V)
    nws = HE.workspace_bytes(T, E, V)
    ws, de = torch.empty(nws, dtype=torch.uint8, device=dev), torch.empty(V, E, dtype=torch.bfloat16, device=dev)
    ours = timed(lambda: HE.embed_bwd(dx, tok, V, 32, -1, d_table=de, workspace=ws), args.warmup, args.reps)
    keep = tok != 32                                                          # (the comparisons get the mask rows zeroed for free)
    acc = torch.zeros(V, E, dtype=torch.float32, device=dev)

    def route_a():
        return acc.zero_().index_add_(0, tok, dx.float()).bfloat16()
    a = timed(route_a, args.warmup, args.reps)
    table = torch.zeros(V, E, dtype=torch.bfloat16, device=dev, requires_grad=True)
    x = torch.nn.functional.embedding(tok, table)

    def route_b():
        return torch.autograd.grad(x, table, dx, retain_graph=True)[0]
    b = timed(route_b, args.warmup, args.reps)
    ref = torch.zeros(V, E, dtype=torch.float64, device=dev).index_add_(0, tok[keep], dx.double()[keep])
    spacing = torch.exp2(torch.floor(torch.log2(ref.abs().clamp(min=1e-30))) - 7)
    off = lambda got: float(((got.double() - ref).abs() / spacing)[torch.arange(V, device=dev) != 32].max())
    moved = T * E * 2 + 2 * nws + V * E * 2
    verdict = 'not slower than (a)' if ours[0] <= a[0] else f'SLOWER than (a) by {100 * (ours[0] / a[0] - 1):.0f} %'
    lines = [f'token-embedding gradient dE[v] = sum of the dX rows of id v; T = {T}, E = {E}, V = {V}, bf16; median of {args.reps} calls after '
             f'{args.warmup} warm-ups, HIP events',
             f'device {torch.cuda.get_device_name(0)}',
             f'ids: proteome-like; largest fan-in {int(counts[4:24].max())} rows (id {int(counts[4:24].argmax()) + 4}), smallest residue fan-in '
             f'{int(counts[4:24].min())}, <cls> {int(counts[0])}, <eos> {int(counts[2])}, <mask> {int(counts[32])} (skipped)',
             f'  esme_hip_embed_bwd                 {ours[0] * 1e3:9.1f} us (min {ours[1] * 1e3:.1f}, max {ours[2] * 1e3:.1f})   {-(-T // HE.ROWS)} chunks of {HE.ROWS} rows, '
             f'workspace {nws / 2 ** 20:.1f} MiB',
             f'      moves {moved / 1e6:.1f} MB (dX once, the partials written and read): {moved / (ours[0] * 1e-3) / 1e12:.2f} TB/s = '
             f'{100 * moved / (ours[0] * 1e-3) / 6.3e12:.0f} % of the ~6.3 TB/s a streaming kernel reaches',
             f'      worst difference from the float64 sum: {off(de):.2f} bf16 spacings',
             f'  (a) fp32 index_add_ + .bfloat16()    {a[0] * 1e3:9.1f} us (min {a[1] * 1e3:.1f}, max {a[2] * 1e3:.1f})   ours / (a) = {ours[0] / a[0]:.3f}  ({verdict})',
             f'      worst difference from the float64 sum: {off(route_a()):.2f} bf16 spacings; two runs bit-equal: {torch.equal(route_a(), route_a())}',
             f'  (b) F.embedding backward in bf16     {b[0] * 1e3:9.1f} us (min {b[1] * 1e3:.1f}, max {b[2] * 1e3:.1f})   ours / (b) = {ours[0] / b[0]:.3f}',
             f'      worst difference from the float64 sum: {off(route_b()):.2f} bf16 spacings; two runs bit-equal: {torch.equal(route_b(), route_b())}']
    if args.step_layers > 0:
        import esme
        from esme import ESM, synthetic as syn
        L, H, n_seq, rows = args.step_layers, 20, 20, 500
        with tempfile.TemporaryDirectory() as td:
            model = ESM.from_pretrained(syn.write_checkpoint(os.path.join(td, 'm.safetensors'), 'esm2_w650', L, E, H, seed=0), device=dev)
        model.train()
        lengths = [rows] * n_seq
        tokens, cu = syn.random_tokens(lengths, 4).to(dev), syn.cu_lens_of(lengths).to(dev)
        mask = torch.rand(tokens.numel(), generator=torch.Generator().manual_seed(2)).lt(0.15).to(dev)
        tokens_in = torch.where(mask, torch.full_like(tokens, model.alphabet.mask_idx), tokens)

        def step():
            model.zero_grad(set_to_none=True)
            logits = model.forward_trainable(tokens_in, (cu, rows), checkpoint_layers=True)
            esme.cross_entropy(logits, tokens, mask, alphabet=model.alphabet).backward()
        w, r = 2, max(5, args.reps // 10)
        model.mark_trainable().mark_lmhead(True)
        off_t = timed(step, w, r)
        model.mark_trainable(embedding=True)
        on_t = timed(step, w, r)
        lines += [f'training step, {L} layers of width {E} (H = {H}), {n_seq} x {rows} rows, masked-token cross entropy, checkpoint_layers=True, everything trainable:',
                  f'  mark_trainable()                    {off_t[0]:8.3f} ms (min {off_t[1]:.3f}, max {off_t[2]:.3f})',
                  f'  mark_trainable(embedding=True)      {on_t[0]:8.3f} ms (min {on_t[1]:.3f}, max {on_t[2]:.3f})   with / without = {on_t[0] / off_t[0]:.4f}']
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
