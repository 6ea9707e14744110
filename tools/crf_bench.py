"""Cost of the linear-chain CRF kernels (esme_hip_crf_fwd / _bwd / _decode) next to a torch-op implementation of the same loss and
Viterbi decoding, timed in the same run on the same box; and the error / bound ratios of every output.

  python tools/crf_bench.py [--reps 10] [--warmup 2] [--out profiles/crf_bench.txt] [--parity profiles/crf_parity.txt]

The torch route is pytorch-crf's data flow: padded (B, S, C) emissions, a (B, S) mask and one step per position (logsumexp over the
previous label for the loss, max / gather for Viterbi), written here.  Both routes compute the negative log-likelihood of fully
labelled sequences (sum) and its gradients with respect to the emissions and the three parameter tensors, and the Viterbi paths.
Shapes: 100 x 500 residues, 13 x 3 846 and 5 000 x 10, at C = 3, 9 and 64.  HIP events, the median of --reps after --warmup (the torch
route with fewer repetitions where one call takes over 100 ms).  Also: how soon the host returns from forward + backward behind 20 ms
of queued work, for both routes; and a training step (loss_trainable -> backward -> AdamW) of a two-layer model of ESM-2 650M's width
with a ResidueCRFHead against the same step with the plain ResidueHead.  --parity: the worst error / bound of every output on the
cases of tests/crf_bounds.py."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'esm-efficient_amd'), os.path.join(ROOT, 'tests')]
DEV = 'cuda:0'


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
    return statistics.median(ts)


def host_return(fn, filler, reps=3):
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


def torch_nll(e, y, mask, A, start, end):
    """sum over sequences of log Z - score(gold) on padded (B, S, C) emissions, (B, S) labels and mask (a prefix per sequence)."""
    B, S, C = e.shape
    idx = torch.arange(B, device=e.device)
    score = start[y[:, 0]] + e[idx, 0, y[:, 0]]
    alpha = start + e[:, 0]
    for t in range(1, S):
        m = mask[:, t]
        score = score + torch.where(m, A[y[:, t - 1], y[:, t]] + e[idx, t, y[:, t]], 0.0)
        nxt = torch.logsumexp(alpha.unsqueeze(2) + A, dim=1) + e[:, t]
        alpha = torch.where(m.unsqueeze(1), nxt, alpha)
    last = y[idx, mask.sum(1) - 1]
    return (torch.logsumexp(alpha + end, dim=1) - (score + end[last])).sum()


def torch_viterbi(e, mask, A, start, end):
    B, S, C = e.shape
    v, back = start + e[:, 0], []
    for t in range(1, S):
        best, arg = (v.unsqueeze(2) + A).max(dim=1)
        m = mask[:, t].unsqueeze(1)
        v = torch.where(m, best + e[:, t], v)
        back.append(torch.where(m, arg, torch.arange(C, device=e.device).expand(B, C)))
    y = (v + end).argmax(1)
    path = [y]
    for arg in reversed(back):
        y = arg.gather(1, y.unsqueeze(1)).squeeze(1)
        path.append(y)
    return torch.stack(path[::-1], 1)


def bench_shape(B, L, C, args, filler, lines):
    from esme.crf import CRF
    g = torch.Generator().manual_seed(B + C)
    T = B * L
    crf = CRF(C).to(DEV).requires_grad_(True)
    e = torch.randn(T, C, generator=g).to(DEV).requires_grad_(True)
    y = torch.randint(0, C, (T,), generator=g).to(DEV)
    cu = (L * torch.arange(B + 1, dtype=torch.int32)).to(DEV)
    chain = torch.ones(T, dtype=torch.bool, device=DEV)
    ep = e.detach().view(B, L, C).clone().requires_grad_(True)
    yp, mask = y.view(B, L), torch.ones(B, L, dtype=torch.bool, device=DEV)
    params = [crf.transitions, crf.start_transitions, crf.end_transitions]

    def ours():
        e.grad = None
        crf.zero_grad(set_to_none=True)
        crf.loss(e, y, cu, chain=chain, reduction='sum').backward()

    def theirs():
        ep.grad = None
        crf.zero_grad(set_to_none=True)
        torch_nll(ep, yp, mask, *params).backward()
    ours()
    l_o, g_o = float(crf.loss(e, y, cu, chain=chain, reduction='sum').detach()), [e.grad.clone()] + [p.grad.clone() for p in params]
    t0 = time.perf_counter()
    theirs()
    torch.cuda.synchronize()
    slow = time.perf_counter() - t0 > 0.1
    l_t = float(torch_nll(ep, yp, mask, *params).detach())
    diffs = [float((a - b).abs().max()) for a, b in zip(g_o, [ep.grad.view(T, C)] + [p.grad for p in params])]
    reps_t, warm_t = (2, 0) if slow else (args.reps, args.warmup)
    o, t = timed(ours, args.warmup, args.reps), timed(theirs, warm_t, reps_t)
    with torch.no_grad():
        do = timed(lambda: crf.decode(e, cu, chain=chain), args.warmup, args.reps)
        dt = timed(lambda: torch_viterbi(ep, mask, *params), warm_t, reps_t)
        same = float((crf.decode(e, cu, chain=chain)[0].view(B, L) == torch_viterbi(ep, mask, *params)).float().mean())
    h_o, h_t = host_return(ours, filler), host_return(theirs, filler)
    verdict = lambda a, b: 'faster' if a <= b else f'SLOWER by {100 * (a / b - 1):.0f} %'
    lines += [f'{B} x {L} residues, C = {C}:',
              f'  loss forward + backward   kernel {o * 1e3:10.1f} us   torch {t * 1e3:12.1f} us   kernel / torch = {o / t:.4f}  ({verdict(o, t)})',
              f'  Viterbi decoding          kernel {do * 1e3:10.1f} us   torch {dt * 1e3:12.1f} us   kernel / torch = {do / dt:.4f}  ({verdict(do, dt)})',
              f'  loss: kernel {l_o:.4f}, torch {l_t:.4f};  largest gradient differences: emissions {diffs[0]:.2e}, transitions {diffs[1]:.2e}, '
              f'start {diffs[2]:.2e}, end {diffs[3]:.2e};  decoded labels equal to torch\'s: {100 * same:.2f} %',
              f'  host returns after forward + backward behind the queued work: kernel route {h_o:.3f} ms, torch route {h_t:.3f} ms']


def training_step(args, lines):
    import esme
    from esme import ESM, synthetic as syn
    from esme.head import ResidueCRFHead, ResidueHead
    from esme.trainer import ResidueModel
    lengths = [200] * 50
    tokens = syn.random_tokens(lengths, 1).to(DEV)
    cu = syn.cu_lens_of(lengths).to(DEV)
    label = torch.randint(0, 3, (tokens.numel(),), generator=torch.Generator().manual_seed(2)).to(DEV)
    label[cu[:-1].long()] = -100
    label[cu[1:].long() - 1] = -100
    out = {}
    for kind in (ResidueHead, ResidueCRFHead):
        with tempfile.TemporaryDirectory() as td:
            model = ESM.from_pretrained(syn.write_checkpoint(os.path.join(td, 'm.safetensors'), 'esm2_t', 2, 1280, 20, seed=0), device=DEV)
        for p in model.parameters():
            p.requires_grad_(False)
        model.add_lora(rank=8, alpha=8, layers=('query', 'value', 'output'))
        model.mark_only_lora_as_trainable()
        net = ResidueModel(model.train(), kind(1280, 3).to(DEV).requires_grad_(True))
        opt = esme.optim.AdamW(net.param_groups(1e-4, 1e-3), weight_decay=0.0)

        def step():
            net.zero_grad(set_to_none=True)
            net.loss_trainable(tokens, (cu, max(lengths)), label).backward()
            opt.step()
        out[kind.__name__] = timed(step, args.warmup + 1, args.reps)
    a, b = out['ResidueHead'], out['ResidueCRFHead']
    lines += [f'training step (two layers of width 1280, LoRA rank 8, 50 x 200 tokens, three labels): ResidueHead {a:.3f} ms, '
              f'ResidueCRFHead {b:.3f} ms (+{b - a:.3f} ms, {100 * (b / a - 1):.1f} %)']


def parity(path):
    import crf_bounds as CB
    from esme import _hip_crf as HC
    lines = ['worst error / bound of every output of the CRF kernels against float64 (tests/crf_bounds.py), per case', f'device {torch.cuda.get_device_name(0)}']
    for case in CB.CASES:
        o = CB.make_case(case)
        ref = CB.reference(*[o[k] for k in ('e', 'A', 'start', 'end', 'cu', 'tags', 'g')], with_bound=True)
        d = {k: v.to(DEV) for k, v in o.items()}
        ops = (d['e'], d['A'], d['start'], d['end'], d['cu'], d['tags'])
        logz, alpha = HC.crf_fwd(*ops)
        de, dA, ds, dn = HC.crf_bwd(*ops, alpha, logz, d['g'])
        p, s = HC.crf_decode(*ops)
        worst = CB.worst_of(dict(logz=logz, de=de, dA=dA, dstart=ds, dend=dn, path=p, score=s), ref, case['kind'] == 'grid')
        lines.append(f"{case['name']:16s} " + '  '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    text = '\n'.join(lines)
    print(text)
    with open(path, 'w') as fh:
        fh.write(text + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default='')
    ap.add_argument('--parity', default='')
    args = ap.parse_args()
    a = torch.randn(4096, 4096, device=DEV, dtype=torch.bfloat16)
    one = timed(lambda: a @ a, 3, 10)
    n_fill = max(1, round(20.0 / one))

    def filler():
        for _ in range(n_fill):
            a @ a
    lines = [f'linear-chain CRF over packed sequences: negative log-likelihood (sum) forward + backward, and Viterbi decoding; float32; median of '
             f'{args.reps} calls after {args.warmup} warm-ups (2 calls where a torch call takes over 100 ms), HIP events',
             f'device {torch.cuda.get_device_name(0)}', f'queued work for the host-return time: {n_fill} x (4096^3 bf16 matmul of {one:.2f} ms) = {n_fill * one:.1f} ms']
    for B, L in ((100, 500), (13, 3846), (5000, 10)):
        for C in (3, 9, 64):
            bench_shape(B, L, C, args, filler, lines)
            print('\n'.join(lines[-5:]), flush=True)
    training_step(args, lines)
    text = '\n'.join(lines)
    print(lines[-1])
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    if args.parity:
        parity(args.parity)


if __name__ == '__main__':
    main()
