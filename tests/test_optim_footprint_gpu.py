"""The device-pointer entry points of include/esme_hip_optim.h inside guard-banded arenas (tests/footprint.py): write containment,
read independence (NaN against zero guards), layout invariance (arena views against contiguous tensors) and an uninitialised, exact-size
workspace -- the discipline tests/test_footprint_gpu.py applies to include/esme_hip.h, with a case list of its own.

The operands are the arrays of the tensors of a list: every one sits in an arena of its own.  The table the entry points read is built
inside `call` from the arena views' addresses and uploaded there; it is not an operand itself (its contents ARE the addresses under
test).  Two tensors of every list are views at an odd element offset (1 and 3), which sends them through the element-wise form, while the
contiguous run of the same case takes the vector form: layout invariance then also says that the two forms agree bit for bit.

Coverage (tests/test_optim_cpu.py fails when a pointer entry point of the header has no case here):

  entry point                      forms covered
  esme_hip_optim_adamw_step        a list of numel 13 (bf16, view at offset 1), CHUNK + 9 (bf16, fp32 gradient: two chunks, ragged tail), 3 (fp32
                                   parameter, view at offset 3), 0 and 2 CHUNK + 5 (bf16); two groups; step counts 1 and 100; param, master,
                                   exp_avg and exp_avg_sq are read and written in place, grad and scale only read
  esme_hip_optim_grad_sqnorm       the same gradients; the exact-size workspace of esme_hip_optim_workspace_bytes, poisoned; clipping active
  esme_hip_optim_grad_accumulate   the same gradients into fp32 accumulators: overwritten (ESME_OPTIM_ACC_INIT: every element written) and
                                   added to
"""
import pytest
import torch

import footprint as fp
import optim_bounds as OB
import test_footprint_gpu as G
from footprint import Case, Operand

pytestmark = pytest.mark.gpu
DEV = G.DEV
CASES = []
C = OB.CHUNK
# (numel, parameter dtype, gradient dtype, group, step count, element offset of the views)
LIST = [(13, G.BF, G.BF, 0, 1, 1), (C + 9, G.BF, G.F32, 1, 100, 0), (3, G.F32, G.F32, 0, 1, 3), (0, G.BF, G.BF, 1, 1, 0), (2 * C + 5, G.BF, G.BF, 0, 100, 0)]
GROUPS = [(1e-3, 0.9, 0.999, 1e-8, 1e-2), (1e-4, 0.9, 0.99, 1e-3, 0.0)]


def add(id, symbols, build):
    CASES.append(G.Spec(id, tuple('esme_hip_' + s for s in symbols.split()), build))


def _operand(name, data, role, off):
    """A 1-D operand; off > 0: a view whose first element lies `off` elements past a 16-byte boundary."""
    if data.numel() == 0:
        data = data.new_zeros(1)                         # (an arena needs a row; the list's numel stays 0 and the row is never touched)
    if not off:
        return Operand(name, data, role)
    return Operand(name, data, role, ld=-(-(data.numel() + 2 * fp.PAD_COLS + 8) // 16) * 16, lead=fp.PAD_COLS + off)


def _tensors(kinds):
    ops = []
    for i, (numel, pdt, gdt, group, t, off) in enumerate(LIST):
        m = G.rnd((numel,), 40 + i, 0.05, G.F32)
        data = dict(param=m.to(pdt), grad=(5e-4 + G.rnd((numel,), 60 + i, 1e-3, G.F32)).to(gdt), master=m, exp_avg=G.rnd((numel,), 80 + i, 3e-4, G.F32),
                    exp_avg_sq=G.rnd((numel,), 90 + i, 1e-3, G.F32) ** 2, acc=G.rnd((numel,), 95 + i, 1e-3, G.F32))
        for kind, role in kinds:
            if kind == 'master' and pdt == G.F32:
                continue                                  # an fp32 parameter is its own master
            ops.append(_operand(f'{kind}{i}', data[kind], role, off))
    return ops


def _table(v, fields, flags=0):
    from esme import _hip_optim as HO
    rows = []
    for i, (numel, pdt, gdt, group, t, off) in enumerate(LIST):
        step_size, isbc2 = HO.bias_terms(GROUPS[group][0], GROUPS[group][1], GROUPS[group][2], t)
        row = dict(numel=numel, group=group, step_size=step_size, inv_sqrt_bc2=isbc2,
                   flags=(HO.PARAM_F32 if pdt == G.F32 else 0) | (HO.GRAD_F32 if gdt == G.F32 else 0) | flags)
        for field, kind in fields.items():
            if f'{kind}{i}' in v:
                row[field] = v[f'{kind}{i}'].data_ptr()
        rows.append(row)
    t = HO.fill_table(rows, [HO.group_record(*g) for g in GROUPS])
    host, dev = HO.upload(t, DEV)
    return t, host, dev


def step_case():
    ops = _tensors([('param', 'inout'), ('grad', 'in'), ('master', 'inout'), ('exp_avg', 'inout'), ('exp_avg_sq', 'inout')])
    ops.append(Operand('scale', torch.tensor([0.37109375]), 'in'))

    def call(v):
        t, host, dev = _table(v, dict(param='param', grad='grad', master='master', exp_avg='exp_avg', exp_avg_sq='exp_avg_sq'))
        G.call_c('esme_hip_optim_adamw_step', host.data_ptr(), dev.data_ptr(), t.n, t.ng, G.P(v['scale']))
    return Case('optim_adamw_step', ops, call)


def sqnorm_case():
    from esme import _hip_optim as HO
    total = int(HO.chunk_prefix([r[0] for r in LIST])[-1])
    nbytes = HO.workspace_bytes(total)
    assert nbytes == 4 * total and total == 2 + 1 + 1 + 3
    ops = _tensors([('grad', 'in')]) + [Operand('ws', torch.empty(nbytes, dtype=torch.uint8), 'ws'), G.out('out', (3,), G.F32, pad=False)]

    def call(v):
        t, host, dev = _table(v, dict(grad='grad'))
        G.call_c('esme_hip_optim_grad_sqnorm', host.data_ptr(), dev.data_ptr(), t.n, t.ng, 1e-3, 0.25, G.P(v['ws']), nbytes, G.P(v['out']))
    return Case('optim_grad_sqnorm', ops, call)


def accumulate_case(init):
    from esme import _hip_optim as HO
    ops = _tensors([('grad', 'in'), ('acc', 'out' if init else 'inout')])
    if init:
        ops = [o for o in ops if not (o.role == 'out' and o.name == 'acc3')]       # (numel 0: nothing is written, so nothing to poison)

    def call(v):
        t, host, dev = _table(v, dict(grad='grad', master='acc'), HO.ACC_INIT if init else 0)
        G.call_c('esme_hip_optim_grad_accumulate', host.data_ptr(), dev.data_ptr(), t.n, t.ng)
    return Case(f'optim_grad_accumulate init={init}', ops, call)


add('optim_adamw_step', 'optim_adamw_step', step_case)
add('optim_grad_sqnorm', 'optim_grad_sqnorm optim_workspace_bytes', sqnorm_case)
add('optim_grad_accumulate-init', 'optim_grad_accumulate', lambda: accumulate_case(True))
add('optim_grad_accumulate-add', 'optim_grad_accumulate', lambda: accumulate_case(False))


@pytest.mark.parametrize('spec', CASES, ids=[c.id for c in CASES])
def test_optim_footprint(spec, monkeypatch):
    from esme import _hip, _hip_optim
    lib, called = _hip.load(), set()
    _hip_optim.bind(lib)                     # (typed on the handle itself: the recorder below hands out plain wrappers)

    class Recorder:
        """The loaded library with every esme_hip_* call noted: the case must reach the entry points its coverage label names."""
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if not name.startswith('esme_hip_') or not callable(fn):
                return fn

            def wrapped(*a):
                called.add(name)
                return fn(*a)
            return wrapped
    monkeypatch.setattr(_hip, '_lib', Recorder())
    case = spec.build()                      # (the builder calls the size query)
    res = fp.check(case, DEV)
    monkeypatch.undo()
    assert set(spec.symbols) <= called, f'{spec.id}: labelled {sorted(spec.symbols)}, but the run called {sorted(called)}'
    # the case itself is sound: every floating-point output holds finite values (bit-equal NaNs would pass the comparisons above)
    for op in case.operands:
        if op.role in ('out', 'inout') and op.data.dtype.is_floating_point:
            assert bool(torch.isfinite(res['nan'].outputs[op.name].view(op.data.dtype).float()).all()), f'{case.name}: output {op.name} is not finite'
    if spec.id == 'optim_adamw_step':        # and it did something: the big tensor's master moved
        before = next(op for op in case.operands if op.name == 'master4').data
        assert not torch.equal(res['nan'].outputs['master4'].view(torch.float32).flatten(), before)
