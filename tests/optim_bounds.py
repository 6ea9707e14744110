"""float64 reference, per-element error bounds and a CPU emulation for the fused AdamW step, the gradient norm and the gradient
accumulator (csrc/optim.hip, include/esme_hip_optim.h).

`reference_step` is the header's arithmetic in float64 on the values the kernel is handed, with the hyperparameters as Python floats.
`step_bound` is the sum of the kernel's rounding steps in units of tests/error_bounds.py's U32 = 2^-24, propagated to first order (a
factor 1 + 2^-10 covers the higher orders): one rounding per fp32 multiply, add, square root and divide, counted as if nothing were
contracted (so it covers the fused and the unfused forms), and one for every host scalar the table carries in fp32 (beta1, 1 - beta1,
beta2, 1 - beta2, eps, 1 - lr wd, lr / bc1, 1 / sqrt(bc2)).  `emulate_step` is a float32 CPU emulation in the kernel's order over a
tensor list, with switches for defects; tests/test_optim_cpu.py checks that the bound accepts the correct emulation and rejects each
defect on the lists and hyperparameters tests/test_optim_gpu.py runs.  `sqnorm_bound` and `accumulate_bound` do the same for the other
two entry points.  Nothing here is tuned to a GPU run.
"""
import math

import torch

import error_bounds as eb

CHUNK = 8192                       # ESME_OPTIM_CHUNK
THREADS, VEC = 256, 8              # kOptThreads, kOptVec (optim.hip)
U = eb.U32
SLACK = 1.0 + 2.0 ** -10
BF, F32 = torch.bfloat16, torch.float32

DEFECTS = ('coupled_decay', 'no_bias_correction', 'eps_inside_sqrt', 'truncated_param', 'master_from_param', 'clip_ignored', 'tail_dropped',
           'next_tensor_overrun', 'shared_step_count')

# Two sets of two groups {lr, betas, eps, weight_decay}: the groups of a set differ in lr, eps and weight_decay; eps takes 1e-8 and 1e-3.
HPS = {
    'a': (dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2), dict(lr=1e-5, betas=(0.9, 0.999), eps=1e-3, weight_decay=1e-1)),
    'b': (dict(lr=1e-4, betas=(0.8, 0.99), eps=1e-3, weight_decay=0.0), dict(lr=3e-3, betas=(0.95, 0.98), eps=1e-8, weight_decay=5e-2)),
}
SCALES = (1.0, 0.37109375)         # the device scalar s (exact in fp32: the kernel reads it from a float): clipping inactive and active

C = CHUNK
# (numel, parameter dtype, gradient dtype, group, steps taken before, element offset of the view, gradient: 'rand' / 'zero' / None)
LISTS = {
    'mixed': [(0, BF, BF, 0, 0, 0, 'rand'), (1, BF, BF, 0, 0, 0, 'rand'), (7, BF, F32, 1, 99, 0, 'rand'), (8, F32, F32, 0, 0, 0, 'rand'),
              (9, BF, BF, 1, 0, 1, 'rand'), (C - 1, BF, BF, 0, 99, 0, 'rand'), (C, F32, F32, 1, 0, 0, 'rand'), (C + 1, BF, F32, 0, 0, 3, 'rand'),
              (100, BF, BF, 0, 5, 0, None), (3 * C + 13, BF, BF, 1, 99, 0, 'rand'), (2 * C + 5, BF, BF, 0, 0, 0, 'zero'),
              (1000, BF, BF, 1, 99, 0, 'zero'), (3 * C + 13, F32, F32, 0, 0, 1, 'rand'), (0, F32, F32, 1, 0, 0, 'rand')],
    'small': [(7, BF, BF, 0, 0, 0, 'rand'), (0, BF, BF, 1, 0, 0, 'rand'), (9, BF, BF, 1, 99, 3, 'rand'), (1, F32, F32, 0, 99, 0, 'rand'), (8, BF, F32, 1, 0, 0, 'rand')],
}


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ the chunk map

def chunk_map(numels):
    """[(tensor, first element, end element)] per chunk, in chunk order: include/esme_hip_optim.h restated in plain Python."""
    out = []
    for r, n in enumerate(numels):
        out += [(r, c * CHUNK, min(n, (c + 1) * CHUNK)) for c in range(_cdiv(n, CHUNK))]
    return out


def find_row(prefix, chunk):
    """opt_find_row of optim.hip: the last r with prefix[r] <= chunk, by bisection; -1 past the list."""
    n = len(prefix) - 1
    if n <= 0 or chunk >= prefix[n]:
        return -1
    lo, hi = 0, n
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if prefix[mid] <= chunk:
            lo = mid
        else:
            hi = mid
    return lo


# ------------------------------------------------------------------ lists

def make_list(name, seed=0):
    """The tensors of LISTS[name] on the CPU: a list of dicts {numel, group, t0, off, pdt, gdt, param, master, m, v, grad}.  Weights
    ~ N(0, 0.05^2), gradients ~ N(5e-4, 1e-3^2); a bf16 parameter is the round-to-nearest-even image of a random fp32 master (so the
    two differ); after steps the moments are random, before the first step zero.  `master` of an fp32 parameter is the parameter."""
    g = torch.Generator().manual_seed(1000 + seed)
    out = []
    for numel, pdt, gdt, group, t0, off, kind in LISTS[name]:
        master = (torch.randn(numel, generator=g) * 0.05).float()
        m = (5e-4 + 3e-4 * torch.randn(numel, generator=g)).float() if t0 else torch.zeros(numel)
        v = (1e-6 * (0.5 + torch.rand(numel, generator=g))).float() if t0 else torch.zeros(numel)
        grad = None
        if kind is not None:
            grad = (5e-4 + 1e-3 * torch.randn(numel, generator=g)).to(gdt) if kind == 'rand' else torch.zeros(numel, dtype=gdt)
        out.append(dict(numel=numel, group=group, t0=t0, off=off, pdt=pdt, gdt=gdt, param=master.to(pdt), master=master, m=m, v=v, grad=grad))
    return out


def stepped(tensors):
    return [t for t in tensors if t['grad'] is not None and t['numel'] > 0]


# ------------------------------------------------------------------ the reference and its bound

def _terms(hp, t):
    lr, (b1, b2), eps, wd = hp['lr'], hp['betas'], hp['eps'], hp['weight_decay']
    return lr, b1, b2, eps, wd, lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t), 1.0 - lr * wd


def reference_step(grad, s, master, m0, v0, hp, t):
    """(w, m, v) float64 after step number t (bias corrections 1 - beta^t) of the header's arithmetic; s: the value of the device scalar."""
    lr, b1, b2, eps, wd, step, isb, decay = _terms(hp, t)
    g = grad.double() * float(s)
    m = b1 * m0.double() + (1.0 - b1) * g
    v = b2 * v0.double() + (1.0 - b2) * g * g
    w = master.double() * decay - step * m / (torch.sqrt(v) * isb + eps)
    return w, m, v


def step_bound(grad, s, master, m0, v0, hp, t):
    """(bound of w, of m, of v) float64 for |kernel - reference_step|."""
    lr, b1, b2, eps, wd, step, isb, decay = _terms(hp, t)
    g = (grad.double() * float(s)).abs()
    m0, v0, w0 = m0.double(), v0.double(), master.double()
    w, m, v = reference_step(grad, s, master, m0, v0, hp, t)
    eg = U * g                                                               # g = float(grad) * s
    em = U * (2 * (b1 * m0).abs() + 2 * (1 - b1) * g + m.abs()) + (1 - b1) * eg        # beta1, the product; 1 - beta1, the product; the sum
    ev = U * (2 * b2 * v0 + 3 * (1 - b2) * g * g + v) + (1 - b2) * 2 * g * eg            # beta2, the product; 1 - beta2, two products; the sum
    r = torch.sqrt(v)
    er = torch.where(v > 0, ev / (2 * torch.clamp(r, min=1e-300)), torch.zeros_like(v)) + U * r             # the square root
    d = r * isb + eps
    ed = er * isb + 2 * U * r * isb + U * eps + U * d                        # 1 / sqrt(bc2), the product; eps; the sum
    q = m / d
    eq = em / d + m.abs() * ed / (d * d) + U * q.abs()                       # the divide
    w1 = w0 * decay
    ew = 2 * U * w1.abs() + 2 * U * (step * q).abs() + step * eq + U * w.abs()           # 1 - lr wd, the product; lr / bc1, the product; the sum
    return ew * SLACK, em * SLACK, ev * SLACK


# ------------------------------------------------------------------ the emulation

def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _f32(x):
    return torch.tensor(float(x), dtype=torch.float64).float()


def rne_bf16(x):
    return x.float().to(BF)


def truncate_bf16(x):
    return (x.float().view(torch.int32) & -65536).view(F32).to(BF)


def _elementwise(gf, s, w, m, v, hp, t, defect):
    lr, b1, b2, eps, wd, step, isb, decay = _terms(hp, t)
    if defect == 'no_bias_correction':
        step, isb = lr, 1.0
    if defect == 'clip_ignored':
        s = 1.0
    g = gf.float() * _f32(s)
    if defect == 'coupled_decay':
        g, decay = g + _f32(wd) * w, 1.0
    m = _fma(_f32(b1), m, _f32(1.0 - b1) * g)
    v = _fma(_f32(b2), v, (_f32(1.0 - b2) * g) * g)
    if defect == 'eps_inside_sqrt':
        d = torch.sqrt(_fma(v, _f32(isb * isb), _f32(eps)))
    else:
        d = _fma(torch.sqrt(v), _f32(isb), _f32(eps))
    w = _fma(-_f32(step), m / d, w * _f32(decay))
    return w, m, v


def emulate_step(tensors, groups, s, defect=None):
    """float32 emulation of esme_hip_optim_adamw_step on the CPU over the list: per tensor a dict {param, master, m, v} after the step
    (the inputs are not modified).  `defect`: None or one of DEFECTS -- 'coupled_decay' (L2 decay added to the gradient),
    'no_bias_correction', 'eps_inside_sqrt', 'truncated_param' (bf16 by truncation), 'master_from_param' (the master re-read from the
    bf16 parameter), 'clip_ignored' (s taken as 1), 'tail_dropped' (the last numel % 8 elements untouched), 'next_tensor_overrun' (a
    ragged last group of 8 runs on into the first elements of the next tensor of the list, as if the arrays were adjacent),
    'shared_step_count' (every tensor corrected with the step count of the first)."""
    assert defect is None or defect in DEFECTS, defect
    outs = [dict(param=t['param'].clone(), master=t['master'].clone(), m=t['m'].clone(), v=t['v'].clone()) for t in tensors]
    live = stepped(tensors)
    t_first = live[0]['t0'] + 1 if live else 1
    for i, t in enumerate(tensors):
        if t['grad'] is None or t['numel'] == 0:
            continue
        o = outs[i]
        step_t = t_first if defect == 'shared_step_count' else t['t0'] + 1
        hp = groups[t['group']]
        n = t['numel'] // VEC * VEC if defect == 'tail_dropped' else t['numel']
        w0 = o['param'].float() if defect == 'master_from_param' and t['pdt'] == BF else o['master']
        w, m, v = _elementwise(t['grad'][:n], s, w0[:n], o['m'][:n], o['v'][:n], hp, step_t, defect)
        o['master'][:n], o['m'][:n], o['v'][:n] = w, m, v
        o['param'][:n] = (truncate_bf16(w) if defect == 'truncated_param' else rne_bf16(w)) if t['pdt'] == BF else w
        if defect == 'next_tensor_overrun' and t['numel'] % VEC:
            nxt = next((j for j in range(i + 1, len(tensors)) if tensors[j]['numel'] > 0), None)
            if nxt is not None:
                k = min(VEC - t['numel'] % VEC, tensors[nxt]['numel'])
                tn, on = tensors[nxt], outs[nxt]
                gn = tn['grad'][:k] if tn['grad'] is not None else torch.zeros(k)
                w, m, v = _elementwise(gn, s, on['master'][:k], on['m'][:k], on['v'][:k], hp, step_t, None)
                on['master'][:k], on['m'][:k], on['v'][:k] = w, m, v
                on['param'][:k] = rne_bf16(w) if tn['pdt'] == BF else w
    return outs


def defect_applies(defect, tensors, groups, s):
    """Whether `defect` changes any output of this list: no decay to couple without weight_decay, nothing to clip at s = 1, bf16
    defects need a bf16 parameter, a tail a numel that is no multiple of 8, an overrun a tensor after such a one, a shared step
    count two different counts."""
    live = stepped(tensors)
    if not live:
        return False
    if defect == 'coupled_decay':
        return any(groups[t['group']]['weight_decay'] > 0 for t in live)
    if defect == 'clip_ignored':
        return s != 1.0 and any(bool(t['grad'].any()) for t in live)
    if defect in ('truncated_param', 'master_from_param'):
        return any(t['pdt'] == BF for t in live)
    if defect == 'tail_dropped':
        return any(t['numel'] % VEC for t in live)
    if defect == 'next_tensor_overrun':
        return any(t['grad'] is not None and t['numel'] % VEC and any(u['numel'] for u in tensors[i + 1:]) for i, t in enumerate(tensors))
    if defect == 'shared_step_count':
        return len({t['t0'] for t in live}) > 1
    return True


def judge(tensors, groups, s, outs):
    """What the tests assert of a step's outputs `outs` (dicts {param, master, m, v} per tensor, any device), as numbers:
    worst = max err / bound over master, m and v of the stepped tensors; param_exact: every bf16 parameter equals the round-to-nearest-even
    image of ITS master bit for bit (an fp32 parameter is its master); untouched: tensors without a gradient are bit-identical."""
    worst, param_exact, untouched = 0.0, True, True
    for t, o in zip(tensors, outs):
        o = {k: x.cpu() for k, x in o.items()}
        if t['grad'] is None or t['numel'] == 0:
            untouched &= all(torch.equal(o[k], t[k]) for k in ('param', 'master', 'm', 'v'))
            continue
        hp, step_t = groups[t['group']], t['t0'] + 1
        ref = reference_step(t['grad'], s, t['master'], t['m'], t['v'], hp, step_t)
        bound = step_bound(t['grad'], s, t['master'], t['m'], t['v'], hp, step_t)
        for got, r, b in zip((o['master'], o['m'], o['v']), ref, bound):
            assert bool(torch.isfinite(got).all()), 'non-finite output'
            err = (got.double() - r).abs()
            worst = max(worst, float(torch.where(err == 0, torch.zeros_like(err), err / b).max()))
        want = rne_bf16(o['master']) if t['pdt'] == BF else o['master']
        param_exact &= o['param'].dtype == want.dtype and torch.equal(o['param'].view(torch.int16 if t['pdt'] == BF else torch.int32),
                                                                      want.view(torch.int16 if t['pdt'] == BF else torch.int32))
    return dict(worst=worst, param_exact=param_exact, untouched=untouched)


def accepted(j):
    return j['worst'] <= 1.0 and j['param_exact'] and j['untouched']


# ------------------------------------------------------------------ the norm and the accumulator

def sqnorm_bound(grads, grad_scale, max_norm):
    """{'norm', 'coef', 'scale'} -> (float64 reference, bound) of out[0..2] of esme_hip_optim_grad_sqnorm for the gradients `grads`
    (tensors; the values the kernel reads).  The squares are non-negative, so every fp32 addition errs by at most U32 of the final sum: a
    lane's chain of CHUNK / 256 fused multiply-adds, 6 butterfly levels, 3 additions over the waves; the float64 pass over the
    partials is counted as one more.  The square root halves the relative error; the conversion to fp32 and grad_scale's own rounding add
    one each; the coefficient adds the sum with 1e-6, the divide and max_norm's rounding, `scale` the last product."""
    S = sum(float((g.double() ** 2).sum()) for g in grads)
    norm = math.sqrt(S) * grad_scale
    rel = (0.5 * (CHUNK // THREADS + 6 + 3 + 1) + 2) * U * SLACK
    coef = 1.0 if max_norm <= 0 else min(1.0, max_norm / (norm + 1e-6))
    rel_c = 0.0 if max_norm <= 0 else rel + 3 * U
    return {'norm': (norm, norm * rel), 'coef': (coef, coef * rel_c), 'scale': (coef * grad_scale, coef * grad_scale * (rel_c + 2 * U))}


def accumulate_bound(micro):
    """(float64 sum, bound) of the fp32 accumulator after adding the gradients `micro` (one tensor per micro-batch) in order: the first
    is copied (exact), every later addition rounds once, by at most U32 of the partial sum."""
    total = micro[0].double().clone()
    bound = torch.zeros_like(total)
    for g in micro[1:]:
        total += g.double()
        bound += U * SLACK * (total.abs() + bound)
    return total, bound
