"""Cost of writing attention maps out: esme_hip_attn_maps next to esme_hip_contact_layer (the same score work, nothing stored) and to
torch materialising the same maps from the same q / k; and model.attention_maps next to the plain forward.

  python tools/attn_maps_bench.py [--reps 20] [--warmup 3] [--out profiles/attn_maps_bench.txt]

The driver starts one child process per step (`--step NAME`), each under a time limit of its own, and stops at the first step that
fails or runs out of time (the report then says which); it does not touch the GPU itself.  Steps:
  kernel-300, kernel-1000     one sequence of 300 / 1 000 rows, H = 20, d = 64, all 20 heads
  kernel-100x500              100 sequences of 500 rows, 2 of the 20 heads
      per step: one esme_hip_attn_maps call in fp32 (with the store bandwidth n_heads * sum S^2 * 4 bytes / time, set against 6.3 TB/s
      of streaming bandwidth), in bf16, and in weighted mode; one esme_hip_contact_layer call on the same operands; and torch's
      softmax((q @ k.T) * scale) per sequence, batched over the selected heads, fp32 -- the only route to the maps without this kernel.
      Device events around `inner` back-to-back calls (a window of milliseconds), the median over --reps windows.
  end-to-end                  synthetic ESM2-650M, 8 x 300 residues: attention_maps(layers=[-1]) and attention_maps(layers=None,
      head_weights='mean') against forward_representation (the one-call forward), forward_representation(layers=[L - 1]) (the per-layer
      module path, which a map request takes too) and predict_contacts, with the peak device memory above the resident state.
Target: one call is no slower than torch's materialisation on any of the three shapes.  A missed target is reported as measured."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'esm-efficient_amd')]
STREAM_TBS = 6.3
STEPS = {'kernel-300': ([300], 20, 240), 'kernel-1000': ([1000], 20, 240), 'kernel-100x500': ([500] * 100, 2, 300), 'end-to-end': (None, None, 600)}
H, D = 20, 64


def windows(fn, warmup, reps, inner):
    """Median, min, max time of one call in ms: device events around `inner` back-to-back calls, `reps` windows after `warmup` calls."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return statistics.median(ts), min(ts), max(ts)


def kernel_step(name, args):
    import torch
    from esme import _hip, _hip_attn_maps as HM, _hip_contacts as HC
    dev = 'cuda:0'
    lengths, n_sel, _ = STEPS[name]
    B, T, E = len(lengths), sum(lengths), H * D
    g = torch.Generator().manual_seed(0)
    qkv = (torch.randn(T, 3 * E, generator=g) * 1.5 ** 0.5).to(torch.bfloat16).to(dev)
    q, k = qkv[:, :E], qkv[:, E:2 * E]
    cu = torch.tensor([0] + torch.tensor(lengths).cumsum(0).tolist(), dtype=torch.int32, device=dev)
    ml, scale = max(lengths), D ** -0.5
    heads = list(range(n_sel))
    hl = torch.tensor(heads, dtype=torch.int32, device=dev)
    hw = torch.full((n_sel,), 1.0 / n_sel, device=dev)
    ws = torch.empty(max(HM.workspace_bytes(B, T, n_sel), 16), dtype=torch.uint8, device=dev)
    S, off, total = HM.map_offsets(cu, n_sel)
    S1, off1, total1 = HM.map_offsets(cu, 1)
    out32, out16 = torch.empty(total, device=dev), torch.empty(total, dtype=torch.bfloat16, device=dev)
    outw = torch.empty(total1, device=dev)
    n, coff, ctotal = HC.map_offsets(cu, 1, 1)
    cmap, cw = torch.empty(ctotal, device=dev), torch.randn(H, generator=g).to(dev)
    cws = torch.empty(HC.workspace_bytes(B, T, H), dtype=torch.uint8, device=dev)
    cul = cu.tolist()

    def torch_maps():
        res = []
        for a, b in zip(cul[:-1], cul[1:]):
            qs, ks = q[a:b].float().view(b - a, H, D)[:, :n_sel], k[a:b].float().view(b - a, H, D)[:, :n_sel]
            res.append(torch.softmax(torch.einsum('ihc,jhc->hij', qs, ks) * scale, dim=2))
        return res

    rows = [('esme_hip_attn_maps fp32', lambda: HM.attn_maps(q, k, cu, ml, H, D, scale, hl, out32, off, 0, ws)),
            ('esme_hip_attn_maps bf16', lambda: HM.attn_maps(q, k, cu, ml, H, D, scale, hl, out16, off, 0, ws)),
            ('esme_hip_attn_maps weighted fp32', lambda: HM.attn_maps(q, k, cu, ml, H, D, scale, hl, outw, off1, 0, ws, head_weights=hw)),
            (f'esme_hip_contact_layer (all {H} heads)', lambda: HC.contact_layer(q, k, cu, ml, H, D, scale, cw, 0.0, True, cmap, coff, cws)),
            ('torch softmax(q k^T * scale), fp32', torch_maps)]
    sq = sum(s * s for s in lengths)
    print(f'{name}: {B} sequence(s) x {ml} rows, H = {H}, d = {D}, {n_sel} head(s) selected; map bytes fp32 {n_sel * sq * 4 / 2 ** 20:.1f} MiB')
    with _hip.stream_scope(dev), torch.no_grad():
        HM.attn_maps(q, k, cu, ml, H, D, scale, hl, out32, off, 0, ws)
        ref = torch_maps()
        err = max(float((out32[o:o + n_sel * s * s].view(n_sel, s, s) - r).abs().max()) for s, o, r in zip(S.tolist(), off.tolist(), ref))
        print(f'  max |esme_hip_attn_maps fp32 - torch fp32| = {err:.3e}')
        del ref
        res = {}
        for label, fn in rows:
            fn()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            inner = max(1, min(200, int(5.0 / max(a.elapsed_time(b), 1e-3))))          # a window of about 5 ms
            res[label] = med, lo, hi = windows(fn, args.warmup, args.reps, inner)
            extra = ''
            if label.startswith('esme_hip_attn_maps'):
                nbytes = (sq if 'weighted' in label else n_sel * sq) * (2 if 'bf16' in label else 4)
                tbs = nbytes / (med * 1e-3) / 1e12
                extra = f'   store {tbs:6.3f} TB/s = {100 * tbs / STREAM_TBS:5.1f} % of {STREAM_TBS} TB/s'
            print(f'  {label:42s} {med * 1e3:10.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}; {inner} calls per window){extra}')
    ours, base = res['esme_hip_attn_maps fp32'][0], res['torch softmax(q k^T * scale), fp32'][0]
    print(f'  esme_hip_attn_maps fp32 / torch = {ours / base:.2f}   target <= 1: {"met" if ours <= base else "MISSED"}')


def end_to_end_step(args):
    import torch
    from esme import ESM, ContactHead, synthetic as syn
    dev = 'cuda:0'
    with tempfile.TemporaryDirectory() as td:
        model = ESM.from_pretrained(syn.write_checkpoint(os.path.join(td, 'm.safetensors'), 'esm2_650m'), device=dev)
    L, Hm = len(model.layers), model.attention_heads
    head = ContactHead(L, Hm)
    head.regression.weight.data.copy_(torch.randn(1, L * Hm, generator=torch.Generator().manual_seed(1)))
    model.set_contact_head(head)
    lengths = [300] * 8
    tokens, cu, ml = syn.random_tokens(lengths, seed=0).to(dev), syn.cu_lens_of(lengths).to(dev), 300
    print(f'end-to-end: ESM2-650M synthetic ({L} layers, {Hm} heads), 8 x 300 residues, precision fast; peak = device memory of one call '
          'above the resident state')
    rows = [('forward_representation (one-call forward)', lambda: model.forward_representation(tokens, (cu, ml))),
            (f'forward_representation(layers=[{L - 1}]) (module path)', lambda: model.forward_representation(tokens, (cu, ml), layers=[L - 1])),
            ('predict_contacts (logits)', lambda: model.predict_contacts(tokens, (cu, ml), logits=True)),
            ('attention_maps(layers=[-1], heads=[0])', lambda: model.attention_maps(tokens, (cu, ml), layers=[-1], heads=[0])),
            ('attention_maps(layers=[-1])', lambda: model.attention_maps(tokens, (cu, ml), layers=[-1])),
            ("attention_maps(layers=None, head_weights='mean')", lambda: model.attention_maps(tokens, (cu, ml), head_weights='mean'))]
    with torch.no_grad():
        for label, fn in rows:
            med, lo, hi = windows(fn, args.warmup, max(5, args.reps // 2), 1)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            print(f'  {label:52s} {med:9.2f} ms  (min {lo:.2f}, max {hi:.2f})   peak {peak / 2 ** 20:8.1f} MiB')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--step', default='')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), 'attn_maps_bench needs a HIP device'
        print(f'device {torch.cuda.get_device_name(0)}; median of {args.reps} windows after {args.warmup} warm-up calls, device events', flush=True) \
            if args.step == 'kernel-300' else None
        end_to_end_step(args) if args.step == 'end-to-end' else kernel_step(args.step, args)
        return 0
    text, rc = [], 0
    for name, (_, _, limit) in STEPS.items():                      # one child per step, each under its own limit; stop at the first failure
        cmd = [sys.executable, os.path.abspath(__file__), '--step', name, '--reps', str(args.reps), '--warmup', str(args.warmup)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
            text.append(done.stdout.rstrip())
            if done.returncode != 0:
                text.append(f'{name}: FAILED with exit status {done.returncode}; the steps after it were not run\n{done.stderr[-2000:]}')
                rc = 1
        except subprocess.TimeoutExpired as e:
            text.append(f'{name}: not finished within its {limit} s limit; the steps after it were not run\n{(e.stdout or b"").decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")}')
            rc = 1
        print(text[-1], flush=True)
        if rc:
            break
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(text) + '\n')
    return rc


if __name__ == '__main__':
    sys.exit(main())
