"""The kernels of include/esme_hip_optim.h on the device against tests/optim_bounds.py: the fused AdamW step, the gradient norm with its
clip coefficient, and the fp32 gradient accumulator, over the tensor lists tests/test_optim_cpu.py vetted the bounds on.

The arrays of a list lie back to back in one pool per kind (parameters, gradients, masters, first and second moments): every tensor
starts at the next 16-byte boundary plus its element offset (0, 1 or 3), so a kernel that runs past a tensor's end lands in its
neighbour or in the few pattern bytes between them, both of which are checked.  The lists mix numel 0, 1, 7, 8, 9, CHUNK - 1, CHUNK,
CHUNK + 1 and 3 CHUNK + 13, bf16 and fp32 parameters and gradients, two groups, step counts 1 and 100, a tensor without a gradient in the
middle, and zero gradients (v = 0: division by eps)."""
import math

import pytest
import torch

import optim_bounds as OB

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KINDS = ('param', 'grad', 'master', 'm', 'v')
PATTERN = 0xA5


def _dtype(t, kind):
    return t['pdt'] if kind == 'param' else t['gdt'] if kind == 'grad' else torch.float32


def place(tensors, kinds=KINDS):
    """({kind: pool}, [{kind: view}]): the list's arrays on the device, back to back in one uint8 pool per kind."""
    spans = {k: [] for k in kinds}
    for kind in kinds:
        cursor = 0
        for t in tensors:
            es = torch.empty(0, dtype=_dtype(t, kind)).element_size()
            held = not (kind == 'master' and t['pdt'] == OB.F32)       # an fp32 parameter is its own master
            a = -(-cursor // 16) * 16 + t['off'] * es
            spans[kind].append((a, a + t['numel'] * es) if held else None)
            if held:
                cursor = a + t['numel'] * es
        spans[kind].append(cursor)
    pools = {k: torch.full((spans[k][-1] + 64,), PATTERN, dtype=torch.uint8, device=DEV) for k in kinds}
    views = []
    for i, t in enumerate(tensors):
        v = {}
        for kind in kinds:
            if spans[kind][i] is None:
                continue
            a, b = spans[kind][i]
            v[kind] = pools[kind][a:b].view(_dtype(t, kind))
            src = t['grad'] if kind == 'grad' else t[kind]
            if src is not None:
                v[kind].copy_(src.to(_dtype(t, kind)))
        views.append(v)
    return pools, views, spans


def outside(pool, spans):
    """the pool's bytes that belong to no tensor"""
    keep = torch.ones(pool.numel(), dtype=torch.bool)
    for s in spans[:-1]:
        if s is not None:
            keep[s[0]:s[1]] = False
    return pool.cpu()[keep]


def run_step(tensors, groups, s):
    from esme import _hip_optim as HO
    pools, views, spans = place(tensors)
    rows, index = [], []
    for i, (t, v) in enumerate(zip(tensors, views)):
        if t['grad'] is None:
            continue
        hp = groups[t['group']]
        step_size, isbc2 = HO.bias_terms(hp['lr'], *hp['betas'], t['t0'] + 1)
        rows.append(dict(param=v['param'].data_ptr(), grad=v['grad'].data_ptr(), master=v['master'].data_ptr() if 'master' in v else 0,
                         exp_avg=v['m'].data_ptr(), exp_avg_sq=v['v'].data_ptr(), numel=t['numel'], group=t['group'], step_size=step_size, inv_sqrt_bc2=isbc2,
                         flags=(HO.PARAM_F32 if t['pdt'] == OB.F32 else 0) | (HO.GRAD_F32 if t['gdt'] == OB.F32 else 0)))
        index.append(i)
    table = HO.fill_table(rows, [HO.group_record(g['lr'], *g['betas'], g['eps'], g['weight_decay']) for g in groups])
    host, dev = HO.upload(table, DEV)
    before = {k: p.clone() for k, p in pools.items()}
    HO.adamw_step(host, dev, table.n, table.ng, torch.tensor([s], dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    outs = [dict(param=v['param'], master=v.get('master', v['param']), m=v['m'], v=v['v']) for v in views]
    return pools, before, spans, outs


@pytest.mark.parametrize('s', OB.SCALES)
@pytest.mark.parametrize('hp', tuple(OB.HPS))
@pytest.mark.parametrize('name', tuple(OB.LISTS))
def test_step_within_bounds(name, hp, s):
    tensors, groups = OB.make_list(name), OB.HPS[hp]
    pools, before, spans, outs = run_step(tensors, groups, s)
    j = OB.judge(tensors, groups, s, outs)
    print(f'\n[optim] {name} hyperparameters {hp} s {s}: worst err / bound {j["worst"]:.3f}')
    assert j['worst'] <= 1.0, j                               # master, exp_avg and exp_avg_sq of every stepped tensor
    assert j['param_exact'], 'a bf16 parameter is not the round-to-nearest-even image of its master'
    assert j['untouched'], 'a tensor without a gradient changed'
    assert torch.equal(pools['grad'], before['grad'])         # gradients are only read
    for k in KINDS:                                           # and nothing between or behind the tensors was written
        assert bool((outside(pools[k], spans[k]) == PATTERN).all()), k
    moved = [float((o['master'].float().cpu() - t['master']).abs().max()) for t, o in zip(tensors, outs) if t['grad'] is not None and t['numel'] > 8 and bool(t['grad'].any())]
    assert min(moved) > 0                                     # (a zero gradient before the first step moves nothing but the decay)
    again = run_step(tensors, groups, s)[0]                   # bit-equal from run to run
    for k in KINDS:
        assert torch.equal(pools[k], again[k]), k


def _grad_table(tensors, views, acc=None, flags=0):
    from esme import _hip_optim as HO
    rows = [dict(grad=v['grad'].data_ptr(), master=acc[i].data_ptr() if acc else 0, numel=t['numel'],
                 flags=(HO.GRAD_F32 if t['gdt'] == OB.F32 else 0) | flags) for i, (t, v) in enumerate(zip(tensors, views))]
    table = HO.fill_table(rows, [])
    return (table,) + HO.upload(table, DEV)


@pytest.mark.parametrize('grad_scale', (1.0, 0.25))
def test_norm_and_clip_coefficient(grad_scale):
    from esme import _hip_optim as HO
    tensors = [t for t in OB.make_list('mixed') if t['grad'] is not None]
    pools, views, spans = place(tensors, ('grad',))
    table, host, dev = _grad_table(tensors, views)
    grads = [t['grad'] for t in tensors]
    before = pools['grad'].clone()
    norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads)) * grad_scale
    need = HO.workspace_bytes(table.total_chunks)
    assert need == 4 * table.total_chunks
    results = {}
    for label, max_norm in (('active', 0.5 * norm), ('inactive', 10.0 * norm), ('off', 0.0)):
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)            # exact size, NaN-poisoned
        out = torch.full((3,), float('nan'), device=DEV)
        HO.grad_sqnorm(host, dev, table.n, 0, max_norm, grad_scale, out, ws)
        got = out.cpu().double()
        want = OB.sqnorm_bound(grads, grad_scale, max_norm)
        for i, k in enumerate(('norm', 'coef', 'scale')):
            ref, bound = want[k]
            print(f'[optim] norm, clipping {label}, grad_scale {grad_scale}: {k} {float(got[i]):.9g} (float64 {ref:.9g}), err / bound '
                  f'{abs(float(got[i]) - ref) / bound if bound else 0.0:.3f}')
            assert abs(float(got[i]) - ref) <= bound, (label, k, float(got[i]), ref, bound)
        results[label] = out.clone()
        out2 = torch.zeros(3, device=DEV)
        HO.grad_sqnorm(host, dev, table.n, 0, max_norm, grad_scale, out2, torch.zeros(need, dtype=torch.uint8, device=DEV))
        assert torch.equal(out, out2)                                            # bit-equal, whatever the workspace held
    assert float(results['active'][1]) < 0.51 and float(results['inactive'][1]) == 1.0 and float(results['off'][1]) == 1.0
    assert torch.equal(pools['grad'], before)                                    # gradients are only read
    # a non-finite norm propagates as in clip_grad_norm_(error_if_nonfinite=False): NaN -> NaN coefficient, inf -> 0
    big = next(v for t, v in zip(tensors, views) if t['numel'] > OB.CHUNK)
    for bad, check in ((float('nan'), math.isnan), (float('inf'), lambda c: c == 0.0)):
        big['grad'][OB.CHUNK] = bad                                 # (the one element of its second chunk)
        out = torch.zeros(3, device=DEV)
        HO.grad_sqnorm(host, dev, table.n, 0, 1.0, grad_scale, out, torch.zeros(need, dtype=torch.uint8, device=DEV))
        assert check(float(out[1])) and not math.isfinite(float(out[0])), (bad, out)


def test_accumulator_after_four_micro_batches():
    from esme import _hip_optim as HO
    base = OB.make_list('mixed')
    micro = [[t for t in OB.make_list('mixed', seed=k) if t['grad'] is not None] for k in range(4)]
    tensors = micro[0]
    apool, aviews, aspans = place([dict(t, pdt=OB.F32, gdt=OB.F32, param=torch.full((t['numel'],), float('nan'))) for t in tensors], ('param',))
    acc = [v['param'] for v in aviews]                                           # uninitialised (NaN) fp32 accumulators, offsets as the list's
    assert len(base) == len(tensors) + 1
    for k, ts in enumerate(micro):
        pools, views, spans = place(ts, ('grad',))
        table, host, dev = _grad_table(ts, views, acc, HO.ACC_INIT if k == 0 else 0)
        HO.grad_accumulate(host, dev, table.n, 0)
        torch.cuda.synchronize()
    worst = 0.0
    for i, a in enumerate(acc):
        ref, bound = OB.accumulate_bound([ts[i]['grad'] for ts in micro])
        err = (a.cpu().double() - ref).abs()
        assert bool((err <= bound).all()), (i, float(err.max()))
        if a.numel():
            assert bool(torch.isfinite(a).all())
            worst = max(worst, float(torch.where(err == 0, torch.zeros_like(err), err / bound).max()))
    print(f'\n[optim] accumulator after 4 micro-batches: worst err / bound {worst:.3f}')
    assert bool((outside(apool['param'], aspans['param']) == PATTERN).all())


class _Recorder:
    """The loaded library with every esme_hip_* call counted by name."""

    def __init__(self, lib):
        self.lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith('esme_hip_') or not callable(fn):
            return fn

        def wrapped(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return wrapped


def _problem(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter((torch.randn(3 + 5 * i, generator=g) * 0.05).to(OB.BF if i % 3 else OB.F32).to(DEV)) for i in range(n)]
    for p in params:
        p.grad = (1e-3 * torch.randn(p.shape, generator=g)).to(p.dtype).to(DEV)
    return params


def test_launch_count_is_independent_of_the_number_of_tensors(monkeypatch):
    import esme
    from esme import _hip, _hip_optim
    lib = _hip.load()
    _hip_optim.bind(lib)
    counts = {}
    for n in (3, 300):
        params = _problem(n)
        opt = esme.optim.AdamW(params, lr=1e-3, max_grad_norm=1.0)
        opt.step()                                            # (state is created here)
        for p in params:
            p.grad = torch.ones_like(p)
        rec = _Recorder(lib)
        monkeypatch.setattr(_hip, '_lib', rec)
        opt.accumulate()
        opt.step()
        monkeypatch.undo()
        torch.cuda.synchronize()
        counts[n] = dict(rec.calls)
    assert counts[3] == counts[300] == {'esme_hip_optim_grad_accumulate': 1, 'esme_hip_optim_workspace_bytes': 1, 'esme_hip_optim_grad_sqnorm': 1,
                                        'esme_hip_optim_adamw_step': 1}, counts


def test_optimiser_steps_like_the_reference():
    """esme.optim.AdamW over 3 steps against float64 AdamW with clip_grad_norm_ on the same gradients: skipped parameters keep their step
    count, the norm is the global one, version counters move, and the masters follow the float64 run."""
    import esme
    params = _problem(7, seed=3)
    shadow = [torch.nn.Parameter(p.detach().double().cpu()) for p in params]
    opt = esme.optim.AdamW([{'params': params[:4]}, {'params': params[4:], 'lr': 1e-4, 'weight_decay': 0.0}], lr=1e-3, max_grad_norm=0.01)
    ref = torch.optim.AdamW([{'params': shadow[:4]}, {'params': shadow[4:], 'lr': 1e-4, 'weight_decay': 0.0}], lr=1e-3)
    g = torch.Generator().manual_seed(11)
    for k in range(3):
        versions = [p._version for p in params]
        for i, (p, q) in enumerate(zip(params, shadow)):
            skip = i == 2 and k == 1
            p.grad = None if skip else (3e-3 * torch.randn(p.shape, generator=g)).to(p.dtype).to(DEV)
            q.grad = None if skip else p.grad.double().cpu()
        want = torch.nn.utils.clip_grad_norm_(shadow, 0.01)
        ref.step()
        opt.step()
        assert abs(float(opt.last_grad_norm) - float(want)) <= 1e-5 * float(want) and opt.last_grad_norm.dim() == 0
        for i, p in enumerate(params):
            assert (p._version > versions[i]) == (p.grad is not None), i
    assert [opt.state[p]['step'] for p in params] == [3, 3, 2, 3, 3, 3, 3]
    for p, q in zip(params, shadow):
        st = opt.state[p]
        assert ('master' in st) == (p.dtype == OB.BF) and st['exp_avg'].dtype == st['exp_avg_sq'].dtype == torch.float32
        w = st['master'] if p.dtype == OB.BF else p.detach()
        # 1e-6: fp32 against float64 arithmetic differs by ~1e-8 at these magnitudes (weights <= 0.2, three steps); a wrong clip coefficient,
        # bias correction, group or step count moves a weight by >= 1e-4 of lr x 3 steps = 3e-3 ... 3e-4
        assert float((w.double().cpu() - q.detach()).abs().max()) <= 1e-6
        if p.dtype == OB.BF:
            assert torch.equal(p.detach(), st['master'].to(OB.BF))
