"""The fused linear + cross-entropy kernel on the device (csrc/linear_xent.hip, include/esme_hip_linear_xent.h): every output of the
forward and the backward against the float64 restatement within the per-element bound of tests/linear_xent_bounds.py, at the smallest
shapes that reach every path (LB.CASES; tests/test_linear_xent_cpu.py shows that the bound rejects the eight defects on them), and
the properties the header states: exact zeros where nothing is kept, out-of-range labels as ignored rows, the dX-only / dW-only flags,
float32 gradients, T == 0, bit-equal runs, rows that do not depend on their batch, no host synchronisation, non-finite rows that stay
where they are, and row offsets past 2^31 elements."""
import pytest
import torch

import linear_xent_bounds as LB

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ARGS = ('x', 'w', 'b', 'y', 'cw', 'g', 'mean')
_SHARED = {}


def run_kernel(o, want_dx=True, want_dw=True, out_f32=False, d_x=None):
    """Forward and backward through the binding: the dict of LB.OUTPUTS."""
    from esme import _hip_linear_xent as HL
    sums, loss_rows, lse = HL.linear_xent_fwd(o['x'], o['w'], o['b'], o['y'], LB.IGNORE, o['cw'], o['mean'])
    dx, dw, db = HL.linear_xent_bwd(o['x'], o['w'], o['b'], o['y'], lse, sums, o['g'], LB.IGNORE, o['cw'], o['mean'], want_dx=want_dx,
                                    want_dw=want_dw, out_f32=out_f32, d_x=d_x)
    return dict(loss=sums[2], L=sums[0], D=sums[1], loss_rows=loss_rows, lse=lse, dx=dx, dw=dw, db=db, sums=sums)


def _case(case):
    """Operands on the device, the float64 reference, the bound and one run of the kernel: computed once per case, shared, never modified."""
    if case['name'] not in _SHARED:
        ops = LB.make_case(case, DEV)
        args = [ops[k] for k in ARGS]
        _SHARED[case['name']] = dict(ops=ops, ref=LB.reference(*args), bound=LB.bound(*args), got=run_kernel(ops))
    return _SHARED[case['name']]


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


@pytest.mark.parametrize('case', LB.CASES, ids=[c['name'] for c in LB.CASES])
def test_outputs_within_the_bound(case):
    c = _case(case)
    got = c['got']
    worst = LB.worst_of(got, c['ref'], c['bound'])
    print(f"{case['name']}: worst err / bound " + ' '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert set(worst) == set(LB.OUTPUTS) - (set() if case['bias'] else {'db'})
    assert max(worst.values()) <= 1.0, worst
    kept = LB._kept(c['ops']['y'], case['C'])
    if case['C'] == 1 or not bool(kept.any()):                                   # one class / nothing kept: the loss and every gradient exactly 0
        assert float(got['loss']) == 0.0 and float(got['L']) == 0.0
        for name in ('loss_rows', 'dx', 'dw', 'db'):
            assert not bool(got[name].any()), name
    if not bool(kept.any()):
        assert float(got['D']) == 0.0
    assert not bool(got['dx'][~kept].any()) and not bool(got['loss_rows'][~kept].any())          # rows that are not kept: zeros


def test_autograd_node_matches_the_kernel_and_scales_with_the_upstream_gradient():
    """esme.loss.linear_cross_entropy on a Linear: (3 * loss).backward() gives the gradients of the kernel run with g = 3, bit for bit,
    in x (a column block of a wider buffer), weight and bias; labels (B, S) against x (B, S, E)."""
    from esme.loss import linear_cross_entropy
    from esme.nn import Linear
    case = next(c for c in LB.CASES if c['name'] == 'T1000-E1280-C33-cw-g3')
    c = _case(case)
    o = c['ops']
    lin = Linear(case['E'], case['C']).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(o['w'])
        lin.bias.copy_(o['b'])
    lin.requires_grad_(True)
    x = o['x'].clone().requires_grad_(True)
    loss = linear_cross_entropy(x.view(10, 100, -1), lin, o['y'].view(10, 100), weight=o['cw'])
    assert loss.dtype == torch.float32 and loss.dim() == 0 and same_bits(loss, c['got']['loss'])
    (3 * loss).backward()
    assert same_bits(x.grad, c['got']['dx']) and same_bits(lin.weight.grad, c['got']['dw']) and same_bits(lin.bias.grad, c['got']['db'])
    ref = torch.nn.functional.cross_entropy(o['x'].float() @ o['w'].float().T + o['b'].float(), o['y'], weight=o['cw'])   # torch's weighted mean
    assert abs(float(loss.detach()) - float(ref)) <= 2 * float(c['bound']['loss'])   # (torch's route on fp32 logits takes the same steps: each is within the bound of the float64 value)
    frozen = Linear(case['E'], case['C']).to(DEV)                                 # a frozen head: only dX
    x2 = o['x'].clone().requires_grad_(True)
    linear_cross_entropy(x2, frozen, o['y']).backward()
    assert x2.grad is not None and frozen.weight.grad is None and frozen.bias.grad is None


def test_out_of_range_labels_are_ignored_rows():
    case = next(c for c in LB.CASES if c['labels'] == 'range')
    c = _case(case)
    y = c['ops']['y']
    assert {-7, case['C'], 2 ** 31 - 1} <= set(y.tolist())
    clean = dict(c['ops'], y=torch.where(LB._kept(y, case['C']), y, torch.full_like(y, LB.IGNORE)))
    got = run_kernel(clean)
    for name in LB.OUTPUTS:
        if c['got'][name] is not None:
            assert same_bits(got[name], c['got'][name]), name


def test_flags_select_the_gradients():
    case = next(c for c in LB.CASES if c['name'] == 'T65-E320-C17-cw-block1')
    c = _case(case)
    full = c['got']
    only_dx = run_kernel(c['ops'], want_dw=False)
    assert only_dx['dw'] is None and only_dx['db'] is None and same_bits(only_dx['dx'], full['dx'])
    only_dw = run_kernel(c['ops'], want_dx=False)
    assert only_dw['dx'] is None and same_bits(only_dw['dw'], full['dw']) and same_bits(only_dw['db'], full['db'])
    f32 = run_kernel(c['ops'], out_f32=True)
    assert f32['dw'].dtype == torch.float32 and f32['db'].dtype == torch.float32
    assert same_bits(f32['dw'].to(torch.bfloat16), full['dw']) and same_bits(f32['db'].to(torch.bfloat16), full['db'])   # the same sums, rounded once
    args = [c['ops'][k] for k in ARGS]
    b32 = LB.bound(*args, out_fmt='fp32')
    worst = LB.worst_of(f32, c['ref'], b32, ('dw', 'db'))
    print('float32 gradients: worst err / bound', worst)
    assert max(worst.values()) <= 1.0
    buf = torch.full((case['T'], 2 * case['E'] + 16), LB.PREFILL, dtype=torch.bfloat16, device=DEV)     # d_x into a column block
    into = run_kernel(c['ops'], d_x=buf[:, 8:8 + case['E']])
    assert same_bits(into['dx'], full['dx']) and bool((buf[:, :8] == LB.PREFILL).all()) and bool((buf[:, 8 + case['E']:] == LB.PREFILL).all())


def test_no_rows():
    o = LB.make_case(dict(name='T0', T=0, E=64, C=3, bias=True, cw=True, mean=True, i64=True, block=None, g=1.0, labels='all'), DEV)
    got = run_kernel(o)
    assert got['sums'].tolist() == [0.0, 0.0, 0.0, 0.0] and got['dx'].shape == (0, 64)
    assert got['dw'].shape == (3, 64) and not bool(got['dw'].any()) and not bool(got['db'].any())


def test_two_runs_are_bit_equal():
    case = next(c for c in LB.CASES if c['name'] == 'T1000-E1280-C33-cw-g3')
    c = _case(case)
    again = run_kernel(c['ops'])
    for name in LB.OUTPUTS:
        assert same_bits(again[name], c['got'][name]), name


def test_a_row_does_not_depend_on_its_batch():
    """Rows run alone (a slice that starts inside a tile and a single row) give the bits of l, lse and dX they have inside the batch."""
    case = next(c for c in LB.CASES if c['name'] == 'T257-E64-C33-i32-cw-sum')
    c = _case(case)
    assert not case['mean']                                                       # (with the mean, dX carries 1 / D of the batch)
    for a, b in ((37, 142), (256, 257), (0, 1)):
        o = dict(c['ops'], x=c['ops']['x'][a:b], y=c['ops']['y'][a:b].clone())
        got = run_kernel(o)
        for name in ('loss_rows', 'lse', 'dx'):
            assert same_bits(got[name], c['got'][name][a:b]), (name, a, b)


def test_forward_and_backward_do_not_synchronise():
    from esme.loss import linear_cross_entropy
    from esme.nn import Linear
    case = next(c for c in LB.CASES if c['name'] == 'T65-E320-C17-cw-block1')
    o = _case(case)['ops']
    lin = Linear(case['E'], case['C']).to(DEV).requires_grad_(True)
    x = o['x'].clone().requires_grad_(True)
    linear_cross_entropy(x, lin, o['y'], weight=o['cw']).backward()               # (the library is loaded and typed)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for reduction in ('mean', 'sum'):
            loss = linear_cross_entropy(x, lin, o['y'], weight=o['cw'], reduction=reduction)
            (loss * 3).backward()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(x.grad.float()).all())


def test_non_finite_rows_stay_where_they_are():
    """A NaN in one kept row of x and a +Inf in another: their l, lse and dX rows, L, the loss, dW and db are non-finite -- never a
    finite number in their place -- and every other row's l, lse and dX keep the bits of the clean run."""
    case = next(c for c in LB.CASES if c['name'] == 'T65-E320-C17-cw-block1')
    c = _case(case)
    kept = LB._kept(c['ops']['y'], case['C']).nonzero().flatten().tolist()
    r_nan, r_inf = kept[1], kept[-1]                                              # (the last row: the partial tile)
    assert r_inf == case['T'] - 1 and r_nan < 64
    buf = c['ops']['buf'].clone()
    x = buf[:, case['E']:]
    x[r_nan, 5] = float('nan')
    x[r_inf, 300] = float('inf')
    got = run_kernel(dict(c['ops'], x=x))
    torch.cuda.synchronize()
    bad = torch.zeros(case['T'], dtype=torch.bool, device=DEV)
    bad[[r_nan, r_inf]] = True
    for name in ('loss_rows', 'lse'):
        assert not bool(torch.isfinite(got[name][bad]).any()), name
        assert same_bits(got[name][~bad], c['got'][name][~bad]), name
    assert not bool(torch.isfinite(got['dx'][bad].float()).any())
    assert same_bits(got['dx'][~bad], c['got']['dx'][~bad])
    for name in ('L', 'loss'):
        assert not bool(torch.isfinite(got[name])), name
    assert float(got['D']) == float(c['got']['D'])                                # (D is a function of the labels alone)
    assert not bool(torch.isfinite(got['db'].float()).any())
    assert not bool(torch.isfinite(got['dw'][:, 5].float()).any()) and not bool(torch.isfinite(got['dw'][:, 300].float()).any())
    assert not bool(torch.isfinite(got['dw'].float()).any())                      # G of the two rows is non-finite in every class


def test_row_offsets_past_2_31_elements():
    """T * ld_x > 2^31 elements (E = 64, C = 2; x a column block of a (T, 4096) buffer): the last rows' l and lse against float64."""
    E, C, ld = 64, 2, 4096
    T = 2 ** 31 // ld + 70
    assert T * ld > 2 ** 31 and T % 64 != 0
    o = LB.make_case(dict(name='big', T=256, E=E, C=C, bias=True, cw=False, mean=False, i64=True, block=None, g=1.0, labels='half'), DEV)
    buf = torch.empty(T, ld, dtype=torch.bfloat16, device=DEV)
    x = buf[:, 128:128 + E]
    x.zero_()
    x[-256:] = o['x']
    y = torch.full((T,), LB.IGNORE, dtype=torch.int64, device=DEV)
    y[-256:] = o['y']
    from esme import _hip_linear_xent as HL
    sums, loss_rows, lse = HL.linear_xent_fwd(x, o['w'], o['b'], y, LB.IGNORE, None, False)
    del buf
    args = [o[k] for k in ARGS]
    ref, bnd = LB.reference(*args), LB.bound(*args)
    got = dict(loss_rows=loss_rows[-256:], lse=lse[-256:])
    worst = LB.worst_of(got, ref, bnd, ('loss_rows', 'lse'))
    print('rows past 2^31 elements: worst err / bound', worst)
    assert max(worst.values()) <= 1.0 and float(ref['loss_rows'].abs().max()) > 0
    assert not bool(loss_rows[:-256].any())                                       # the ignored rows: zeros
    b64 = o['b'].double()
    assert abs(float(lse[0]) - float(torch.logsumexp(b64, 0))) < 1e-6             # a zero row: lse of the bias
    tail = float(ref['L'])
    assert abs(float(sums[0]) - tail) <= float(bnd['L']) + LB.gamma(T) * abs(tail)
