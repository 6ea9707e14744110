"""GPU tests of the attention-pooling backward (csrc/pool_bwd.hip, include/esme_hip_attn_pool_bwd.h).

The kernel is judged per element against float64 autograd through the folded definition, |got - ref64| <= bound for dX and for dU with
no rms floor (tests/attn_pool_bwd_bounds.py: the bound is the sum of the kernel's rounding steps and is vetted on the CPU against an
emulation with defects, tests/test_attn_pool_bwd_cpu.py), on the smallest shapes at which it can go wrong, in bf16 and in fp32; then
the reproducibility contract of the header, and the fold kernel against esme.autograd.pool_fold."""
import math

import pytest
import torch

import attn_pool_bounds as apb
import attn_pool_bwd_bounds as PB
from error_bounds import C_DOT, U32, assert_bounded

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = {'bf16': torch.bfloat16, 'fp32': torch.float32}
_SHARED = {}


def _bwd(c, **kw):
    from esme import _hip_attn_pool_bwd as HB
    return HB.attn_pool_bwd(c['x'], c['cu'], c['U'], c['d_out'], c['heads'], c['n_cls'], **kw)


def _case(i, fmt):
    """Operands on the device, one kernel run, the float64 reference and the bound: computed once, shared, never modified."""
    if (i, fmt) not in _SHARED:
        lengths, E, H, C = PB.SHAPES[i]
        c = PB.make_operands(lengths, E, H, C, DTYPES[fmt], seed=7 + i, device=DEV)
        ref = PB.reference_pool_grads(c['x'], c['cu'], c['U'], c['d_out'], H)
        _SHARED[i, fmt] = dict(c, ref=ref, bound=PB.pool_bwd_bound(c['x'], c['cu'], c['U'], c['d_out'], H, ref[0], fmt), got=_bwd(c))
    return _SHARED[i, fmt]


CASES = [(i, fmt) for i in range(len(PB.SHAPES)) for fmt in ('bf16', 'fp32')]


@pytest.mark.parametrize('i,fmt', CASES)
def test_gradients_within_bound(i, fmt):
    c = _case(i, fmt)
    dx, dU = c['got']
    assert dx.dtype == DTYPES[fmt] and dx.shape == c['x'].shape and dU.dtype == torch.float32 and dU.shape == c['U'].shape
    wx = assert_bounded(dx, c['ref'][0], c['bound'][0], f'attn_pool_bwd dX shape {i} {fmt}')
    wu = assert_bounded(dU, c['ref'][1], c['bound'][1], f'attn_pool_bwd dU shape {i} {fmt}')
    print(f'shape {i} {fmt}: worst err / bound dX {wx:.3f} dU {wu:.3f}')


@pytest.mark.parametrize('i,fmt', CASES)
def test_without_dx_and_run_to_run(i, fmt):
    c = _case(i, fmt)
    dx, dU = c['got']
    none, dU0 = _bwd(c, need_dx=False)
    assert none is None and torch.equal(dU0, dU)                         # dU does not depend on whether dx was asked for
    dx2, dU2 = _bwd(c)
    assert torch.equal(dx2, dx) and torch.equal(dU2, dU)                 # two runs are bit-equal


@pytest.mark.parametrize('i,fmt', CASES)
def test_each_sequence_alone_is_bit_equal(i, fmt):
    c = _case(i, fmt)
    dx = c['got'][0]
    cu = c['cu'].tolist()
    for s in range(len(cu) - 1):
        a, b = cu[s], cu[s + 1]
        if a == b:
            continue
        one = dict(c, x=c['x'][a:b].contiguous(), d_out=c['d_out'][s:s + 1].contiguous(), cu=torch.tensor([0, b - a], dtype=torch.int32, device=DEV))
        assert torch.equal(_bwd(one)[0], dx[a:b]), f'sequence {s} (rows {a}..{b})'


@pytest.mark.parametrize('fmt', ('bf16', 'fp32'))
def test_zero_d_out_gives_exact_zeros(fmt):
    c = _case(1, fmt)
    dx, dU = _bwd(dict(c, d_out=torch.zeros_like(c['d_out'])))
    assert not bool(dx.any()) and not bool(dU.any())


def test_rows_outside_the_sequences_are_left_alone():
    """cu_lens that starts past row 0 and ends before row T: the rows of dx that belong to no sequence keep what the caller passed; an
    all-empty batch gives dU = 0."""
    c = _case(2, 'bf16')
    T, E = c['x'].shape
    x = torch.cat([c['x'][:3], c['x'], c['x'][:2]])
    cu = (c['cu'] + 3).to(torch.int32)
    dx = torch.full((T + 5, E), 7.0, dtype=torch.bfloat16, device=DEV)
    got, dU = _bwd(dict(c, x=x, cu=cu), dx=dx)
    assert bool((got[:3] == 7).all()) and bool((got[T + 3:] == 7).all())
    assert torch.equal(got[3:T + 3], c['got'][0]) and torch.equal(dU, c['got'][1])
    empty = dict(c, cu=torch.zeros(3, dtype=torch.int32, device=DEV), d_out=c['d_out'][:2].contiguous())
    dx0, dU0 = _bwd(empty)
    assert not bool(dx0.any()) and not bool(dU0.any())


def test_fold_kernel_agrees_with_pool_fold():
    """esme_hip_attn_pool_fold against esme.autograd.pool_fold: both within the fold's fp32 rounding of float64, so within twice that
    of each other."""
    from esme import _hip
    from esme.autograd import pool_fold
    g = torch.Generator().manual_seed(9)
    for C, H, E in ((1, 4, 64), (3, 5, 40), (2, 20, 1280)):
        d = E // H
        cls = torch.randn(C, E, generator=g).to(torch.bfloat16).to(DEV)
        wk = (torch.randn(E, E, generator=g) / math.sqrt(E)).to(torch.bfloat16).to(DEV)
        got, tor = _hip.attn_pool_fold(cls, wk, H), pool_fold(cls, wk, H)
        assert got.shape == tor.shape and tor.dtype == torch.float32
        scale = apb.LOG2E / math.sqrt(d)
        qh, Wh = cls.double().view(C, H, d), wk.double().view(H, d, E)
        ref = (scale * torch.einsum('chd,hde->che', qh, Wh)).reshape(C * H, E)
        bound = (scale * C_DOT * U32 * math.sqrt(d) * torch.sqrt(torch.einsum('chd,hde->che', qh * qh, Wh * Wh)).reshape(C * H, E)
                 + 2 * U32 * ref.abs())
        assert_bounded(got, ref, bound, f'attn_pool_fold kernel C={C} H={H} E={E}')
        assert_bounded(tor, ref, bound, f'pool_fold torch C={C} H={H} E={E}')
        assert_bounded(got, tor.double(), 2 * bound, f'kernel against pool_fold C={C} H={H} E={E}')
