"""Cost of predict_contacts next to the plain forward and to a torch implementation that materialises every attention map.

  python tools/contacts_bench.py [--reps 10] [--warmup 3] [--out profiles/contacts_bench.txt]

ESM2-650M geometry (33 layers, E = 1 280, H = 20) with synthetic weights and a random contact regression, 100 sequences of 500
residues, precision 'fast'.  HIP events around each call, the median of --reps steps after --warmup, and the peak device memory of one
step above what was allocated before it, for
  * model.predict_contacts (one esme_hip_contact_layer call per layer; logits);
  * model.forward_representation on the same batch;
  * the definition in plain torch on the GPU, from the per-layer q / k that predict_contacts captured (the forward itself is NOT
    in this figure): per sequence an einsum of scores, softmax, the (H, n, n) maps of every layer materialised, APC and the regression.
There is no pass mark.  The expectation to compare against: about four Q K^T products per layer against attention's two products,
i.e. 1.5 - 2 x the attention kernel's FLOPs, with attention about 10 % of the forward.  Where predict_contacts comes out above
2 x the plain forward, one `rocprofv3 --kernel-trace --stats -- python tools/contacts_bench.py --reps 3 --skip-torch` run says where the time goes."""
import argparse
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'esm-efficient_amd')]
LOG2E = 1.4426950408889634


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
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return statistics.median(ts), min(ts), max(ts), peak


def torch_contacts(qk, cu, H, d, scale, w, bias):
    """The definition with every map materialised: per sequence, (L, H, n, n) fp32 features, then the regression."""
    cul = cu.tolist()
    out = []
    for a, b in zip(cul[:-1], cul[1:]):
        S = b - a
        feats = []
        for _, q, k, qp in qk:
            qs, ks = q[a:b].float().view(S, H, d), k[a:b].float().view(S, H, d)
            s = torch.einsum('ihc,jhc->hij', qs, ks) * (1.0 / LOG2E if qp else scale)
            A = torch.softmax(s, dim=2)[:, 1:S - 1, 1:S - 1]
            Y = A + A.transpose(1, 2)
            r = Y.sum(2)
            feats.append(Y - r[:, :, None] * r[:, None, :] / r.sum(1)[:, None, None])
        feats = torch.stack(feats)                                   # (L, H, n, n)
        out.append(bias + torch.einsum('lh,lhij->ij', w, feats))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--skip-torch', action='store_true')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    from esme import ESM, ContactHead, synthetic as syn
    dev = 'cuda:0'
    with tempfile.TemporaryDirectory() as td:
        model = ESM.from_pretrained(syn.write_checkpoint(os.path.join(td, 'm.safetensors'), 'esm2_650m'), device=dev)
    L, H = len(model.layers), model.attention_heads
    head = ContactHead(L, H)
    head.regression.weight.data.copy_(torch.randn(1, L * H, generator=torch.Generator().manual_seed(1)))
    model.set_contact_head(head)
    tokens, cu, max_len, _ = syn.uniform_batch(50000, 500, seed=0)
    tokens, cu = tokens.to(dev), cu.to(dev)
    lines = [f'ESM2-650M synthetic, {cu.numel() - 1} sequences x {max_len} residues ({tokens.numel()} rows), precision fast; '
             f'median of {args.reps} after {args.warmup} warm-ups, HIP events; peak = device memory of one step above the resident state',
             f'device {torch.cuda.get_device_name(0)}']
    with torch.no_grad():
        rows = [('predict_contacts (logits)', lambda: model.predict_contacts(tokens, (cu, max_len), logits=True)),
                ('forward_representation', lambda: model.forward_representation(tokens, (cu, max_len)))]
        res = {}
        for name, fn in rows:
            res[name] = timed(fn, args.warmup, args.reps)
        if not args.skip_torch:
            ours = model.predict_contacts(tokens, (cu, max_len), logits=True, _keep_qk=True)
            qk = model._contact_qk
            w = model.contact_head.regression.weight.detach().reshape(L, H)
            d, scale = model.head_pad, (model.embed_dim // H) ** -0.5
            fn = lambda: torch_contacts(qk, cu, H, d, scale, w, 0.0)
            res['torch, maps materialised (q / k given)'] = timed(fn, 1, max(3, args.reps // 3))
            ref = fn()
            err = max(float((a - b).abs().max()) for a, b in zip(ours, ref))
            lines.append(f'max |predict_contacts - torch fp32| over the batch: {err:.3e}')
    for name, (med, lo, hi, peak) in res.items():
        lines.append(f'{name:42s} {med:9.2f} ms  (min {lo:.2f}, max {hi:.2f})   peak {peak / 2 ** 20:9.1f} MiB')
    pc, fw = res['predict_contacts (logits)'][0], res['forward_representation'][0]
    lines.append(f'predict_contacts / forward_representation = {pc / fw:.2f}   (contact kernels: {pc - fw:.2f} ms = {(pc - fw) / L * 1e3:.0f} us per layer)')
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
