"""The attention-pooling backward without a GPU: the error bound of tests/attn_pool_bwd_bounds.py accepts a float32 emulation of the
kernel and rejects every defect the emulation can switch on, on the shapes tests/test_attn_pool_bwd_gpu.py runs; the host-side
argument checks of the entry points through the cross-compiled library; the bookkeeping of the new header (footprint coverage,
binding table, exported symbols); and what the heads' forward_trainable rests on that needs no device."""
import ctypes
import math
import os
import re

import pytest
import torch

import attn_pool_bounds as apb
import attn_pool_bwd_bounds as PB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'esme_hip_attn_pool_bwd.h')
DTYPES = {'bf16': torch.bfloat16, 'fp32': torch.float32}
_SHARED = {}


def _case(i, fmt):
    """One batch, its float64 reference and bound: computed once per (shape, dtype), shared, never modified."""
    if (i, fmt) not in _SHARED:
        lengths, E, H, C = PB.SHAPES[i]
        c = PB.make_operands(lengths, E, H, C, DTYPES[fmt], seed=7 + i)
        ref = PB.reference_pool_grads(c['x'], c['cu'], c['U'], c['d_out'], H)
        _SHARED[i, fmt] = dict(c, ref=ref, bound=PB.pool_bwd_bound(c['x'], c['cu'], c['U'], c['d_out'], H, ref[0], fmt))
    return _SHARED[i, fmt]


def _emulate(c, defect=None, need_dx=True):
    return PB.emulate_pool_bwd(c['x'], c['cu'], c['U'], c['d_out'], c['heads'], defect=defect, need_dx=need_dx)


def test_reference_equals_the_stated_formulas():
    """float64 autograd through the folded definition equals the issue's closed form (dP, Delta, dsigma, dU, dX)."""
    c = PB.make_operands((5, 0, 70), 16, 2, 3, torch.float32, seed=1)
    x, U, g, H = c['x'].double(), c['U'].double(), c['d_out'].double(), 2
    C, d, E = 3, 8, 16
    dX, dU = PB.reference_pool_grads(c['x'], c['cu'], c['U'], c['d_out'], H)
    eX, eU = torch.zeros_like(dX), torch.zeros_like(dU)
    for s, (a, b) in enumerate(((0, 5), (5, 5), (5, 75))):
        if a == b:
            continue
        xs = x[a:b]
        p = torch.softmax(PB.LN2 * xs @ U.T, 0)
        dP = torch.einsum('thd,chd->tch', xs.view(-1, H, d), g[s].view(C, H, d)).reshape(-1, C * H)
        dsig = PB.LN2 * p * (dP - (p * dP).sum(0))
        eU += dsig.T @ xs
        eX[a:b] = dsig @ U + (p.view(-1, C, H).repeat_interleave(d, 2) * g[s]).sum(1)
    assert float((dX - eX).abs().max()) < 1e-12 and float((dU - eU).abs().max()) < 1e-12


@pytest.mark.parametrize('fmt', ('bf16', 'fp32'))
@pytest.mark.parametrize('i', range(len(PB.SHAPES)))
def test_bound_accepts_the_correct_emulation(i, fmt):
    c = _case(i, fmt)
    worst = PB.worst(_emulate(c), c['ref'], c['bound'])
    print(f'shape {i} {fmt} correct emulation: worst err / bound {worst:.3f}')
    assert worst <= 1.0
    for r, b in zip(c['ref'], c['bound']):                     # the bound resolves the signal: the largest gradient is far above the largest bound
        assert float(r.abs().max()) >= 20 * float(b.max())
    dx0, du0 = _emulate(c, need_dx=False)
    assert dx0 is None and torch.equal(du0, _emulate(c)[1])


@pytest.mark.parametrize('fmt', ('bf16', 'fp32'))
@pytest.mark.parametrize('i', range(len(PB.SHAPES)))
@pytest.mark.parametrize('defect', PB.DEFECTS)
def test_bound_rejects_every_defect(defect, i, fmt):
    c = _case(i, fmt)
    worst = PB.worst(_emulate(c, defect), c['ref'], c['bound'])
    print(f'shape {i} {fmt} {defect}: worst err / bound {worst:.1f}')
    assert worst > 1.0, f'the bound accepts the defect {defect!r}'


def test_zero_d_out_and_empty_batch():
    c = PB.make_operands((3, 0, 66), 16, 2, 1, torch.bfloat16, seed=2)
    dx, du = PB.emulate_pool_bwd(c['x'], c['cu'], c['U'], torch.zeros_like(c['d_out']), 2)
    assert not dx.any() and not du.any()
    rx, ru = PB.reference_pool_grads(c['x'], c['cu'], c['U'], torch.zeros_like(c['d_out']), 2)
    assert not rx.any() and not ru.any()


# ------------------------------------------------------------------ the header's bookkeeping

def _declared():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r'\b(esme_hip_\w+)\s*\(([^;{}]*?)\)\s*;', text)}


def test_every_pointer_entry_point_has_a_footprint_case():
    import test_attn_pool_bwd_footprint_gpu as G
    names = [n for n, args in _declared().items() if '*' in args]
    assert names == ['esme_hip_attn_pool_bwd']
    covered = {s for c in G.CASES for s in c.symbols}
    for n in names:
        assert n in covered, f'{n}: declared in esme_hip_attn_pool_bwd.h with a pointer argument, but no case in tests/test_attn_pool_bwd_footprint_gpu.py names it'
        assert re.search(rf'\b{n}\b', G.__doc__), f'{n}: missing from the docstring of tests/test_attn_pool_bwd_footprint_gpu.py'
    assert covered <= set(_declared()), covered - set(_declared())
    ids = [c.id for c in G.CASES]
    assert len(ids) == len(set(ids))
    assert any('nodx' in i for i in ids) and any('nodx' not in i for i in ids)      # dx present and NULL


def test_header_symbols_exported_and_bound():
    from esme import _hip, _hip_attn_pool_bwd
    declared = set(_declared())
    assert declared == set(_hip_attn_pool_bwd.SIGNATURES) == {'esme_hip_attn_pool_bwd_workspace_bytes', 'esme_hip_attn_pool_bwd'}
    lib = ctypes.CDLL(_hip.lib_path())
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/esme_hip_attn_pool_bwd.h but not exported'
    assert not declared & set(_hip.SIGNATURES)                                   # the main table and header keep their own symbols
    assert 'esme_hip_attn_pool_bwd' not in open(os.path.join(ROOT, 'include', 'esme_hip.h')).read()
    for name, args in _declared().items():                                       # the number of arguments of each declaration equals the binding's
        assert len([a for a in args.split(',') if a.strip()]) == len(_hip_attn_pool_bwd.SIGNATURES[name][1]), name
    mk = open(os.path.join(ROOT, 'esm-efficient_amd', 'csrc', 'Makefile')).read()
    assert 'pool_bwd.hip' in mk and 'esme_hip_attn_pool_bwd.h' in mk


def test_host_validation_of_the_entry_points():
    """Host-side checks need no device: the size query's stated formula and geometry errors, and the argument errors that return
    before any launch."""
    from esme import _hip_attn_pool_bwd as HB
    slot = lambda J, E: 2 + 3 * J + 2 * 64 * J + J * E
    assert HB.workspace_bytes(2, 100, 256, 4, 1) == (2 + 1 + 1) * slot(4, 256) * 4
    assert HB.workspace_bytes(100, 50000, 1280, 20, 4) == (100 + 781 + 1) * slot(80, 1280) * 4
    assert HB.workspace_bytes(2, 100, 1280, 32, 16) == (2 + 1 + 1) * slot(512, 1280) * 4
    lib = HB._lib()
    q = lib.esme_hip_attn_pool_bwd_workspace_bytes
    assert q(2, 100, 256, 3, 1) == -1 and b'multiple of heads' in lib.esme_hip_last_error()       # E % heads
    assert q(2, 100, 36, 4, 1) == -1                                             # E % 8
    assert q(-1, 100, 256, 4, 1) == -1 and q(2, -1, 256, 4, 1) == -1 and q(2, 100, 256, 4, 0) == -1
    assert q(2, 100, 1280, 20, 26) == -2 and b'n_cls * heads > 512' in lib.esme_hip_last_error()   # J = 520
    with pytest.raises(RuntimeError, match='code -2'):
        HB.workspace_bytes(2, 100, 1280, 20, 26)
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    need = HB.workspace_bytes(2, 10, 256, 4, 1)
    args = dict(x=p, ldx=256, cu=p, B=2, T=10, E=256, H=4, C=1, U=p, g=p, ldg=256, dx=p, lddx=256, dU=p, ws=p, nb=need, f32=0, stream=None)
    call = lambda **kw: lib.esme_hip_attn_pool_bwd(*{**args, **kw}.values())
    for bad in (dict(x=None), dict(cu=None), dict(U=None), dict(g=None), dict(dU=None), dict(ws=None),            # null pointers
                dict(x=p + 8), dict(U=p + 4), dict(dx=p + 2), dict(ws=p + 8),                                     # misaligned
                dict(ldx=260), dict(ldx=258, f32=1), dict(lddx=260), dict(ldx=128), dict(lddx=128), dict(ldg=128), dict(C=2),    # strides (C = 2: ldg < n_cls E)
                dict(nb=need - 1), dict(nb=0),                                                                    # a short workspace
                dict(E=250, H=5, ldx=256), dict(E=256, H=3), dict(B=-1), dict(T=-1), dict(C=0)):                  # geometry
        assert call(**bad) == -1, bad
    assert call(nb=need - 1) == -1 and b'workspace too small' in lib.esme_hip_last_error()
    assert call(E=1280, H=20, C=26, ldx=1280, lddx=1280, ldg=26 * 1280, nb=1 << 40) == -2                        # J > 512
    assert call(dx=None, lddx=0, nb=need - 1) == -1                                # (dx = NULL is legal: the next refusal is the workspace's)


# ------------------------------------------------------------------ Python-level behaviour that needs no device

def test_heads_still_construct_frozen_and_have_forward_trainable():
    from esme.head import ClsHead
    from esme.pooling import AttentionPool, BinaryLearnedAggregation, LearnedAggregation, LearnedAttentionPool
    for m in (AttentionPool(4, 64), LearnedAttentionPool(2, 4, 64), LearnedAggregation(3, 4, 64), BinaryLearnedAggregation(4, 64), ClsHead(64, 2, 128)):
        assert all(not p.requires_grad and p.dtype == torch.bfloat16 for p in m.parameters()), type(m).__name__
        assert callable(getattr(m, 'forward_trainable')), type(m).__name__
        m.requires_grad_(True)                                                   # the opt-in
        assert all(p.requires_grad for p in m.parameters())
    with pytest.raises(NotImplementedError):
        BinaryLearnedAggregation(4, 64, dropout_p=0.1)
    with pytest.raises(TypeError):
        BinaryLearnedAggregation(4, 64).forward_trainable(torch.ones(3, 64, dtype=torch.float16), (torch.tensor([0, 3]), 3))
    with pytest.raises(TypeError):
        ClsHead(64, 2, 128).forward_trainable(torch.ones(3, 64, dtype=torch.float16), torch.tensor([0, 3]))
    with pytest.raises(NotImplementedError, match='forward_trainable'):
        BinaryLearnedAggregation(4, 64).float().forward_trainable(torch.ones(3, 64), (torch.tensor([0, 3]), 3))


def test_pool_fold_equals_the_float64_fold():
    """esme.autograd.pool_fold against float64 within the fold's fp32 rounding ([fold-scale] of attn_pool_bounds.pool_bound), and
    differentiable in cls and k.weight."""
    from esme.autograd import pool_fold
    from error_bounds import C_DOT, U32
    g = torch.Generator().manual_seed(5)
    C, H, E = 3, 5, 40
    d = E // H
    cls = torch.randn(C, E, generator=g).to(torch.bfloat16).requires_grad_()
    wk = (torch.randn(E, E, generator=g) / math.sqrt(E)).to(torch.bfloat16).requires_grad_()
    U = pool_fold(cls, wk, H)
    assert U.dtype == torch.float32 and U.shape == (C * H, E)
    scale = apb.LOG2E / math.sqrt(d)
    qh, Wh = cls.detach().double().view(C, H, d), wk.detach().double().view(H, d, E)
    ref = scale * torch.einsum('chd,hde->che', qh, Wh)
    bound = scale * C_DOT * U32 * math.sqrt(d) * torch.sqrt(torch.einsum('chd,hde->che', qh * qh, Wh * Wh)) + 2 * U32 * ref.abs()
    assert bool(((U.detach().double().view(C, H, E) - ref).abs() <= bound).all())
    U.sum().backward()
    assert cls.grad is not None and wk.grad is not None and cls.grad.dtype == torch.bfloat16
    # d(sum U) / d cls[c, h d + i] = scale * sum_e W[h d + i, e]
    want = (scale * wk.detach().double().sum(1)).expand(C, E)
    assert float((cls.grad.double() - want).abs().max()) <= 2.0 ** -7 * float(want.abs().max())


def test_k_bias_has_zero_gradient_in_float64():
    """The reference's data flow keeps the key bias (attn_pool_bounds.reference_pool); it adds a constant to every score of a
    (class token, head) and cancels in the softmax, so its gradient is zero: what justifies forward_trainable giving it none."""
    g = torch.Generator().manual_seed(6)
    E, H, C = 32, 4, 2
    x = torch.randn(75, E, generator=g).double().requires_grad_()
    cls = torch.randn(C, E, generator=g).double().requires_grad_()
    wk = (torch.randn(E, E, generator=g) / math.sqrt(E)).double().requires_grad_()
    bk = torch.randn(E, generator=g).double().requires_grad_()
    out, _ = apb.reference_pool(x, torch.tensor([0, 5, 75]), cls, wk, bk, H)
    (out * torch.randn(out.shape, generator=g).double()).sum().backward()
    assert float(wk.grad.abs().max()) > 1e-3 and float(cls.grad.abs().max()) > 1e-3
    assert float(bk.grad.abs().max()) <= 1e-12 * float(wk.grad.abs().max())
