"""GPU tests of the position-table gradient (csrc/embed_positions_bwd.hip, include/esme_hip_embed_positions_bwd.h).

The kernel is judged per element against float64, |got - ref64| <= bound with no rms floor (tests/embed_positions_bwd_bounds.py: the
bound is the sum of the kernel's rounding steps and is vetted on the CPU against an emulation with defects,
tests/test_embed_positions_bwd_cpu.py), at E in {64, 320} x six length patterns (one sequence; three of one row; empty sequences first
and in the middle; 33 / 1 / 64 / 2 / 65 rows; 65 sequences of 1 .. 70 rows, i.e. nine rounds of the kernel's eight sequences in flight;
300 sequences of three rows) x P in {max_len + 2, max_len + 40}, pos_offset 2, then pos_offset 0 and a max_len below the longest
sequence.  Every case runs on a contiguous dX and on a column view of a wider buffer (a padded row stride), into a table that held 7.0:
the rows nothing reaches must be exact zeros.  The result is bit-equal to the float32 emulation of the header's order, from run to run,
and doubling one sequence's rows doubles exactly the table rows it alone reaches.  Then B = 0 and T = 0, the refusals, 70 002 sequences
and a d_x whose rows pass element 2^31 (the two limits tests/test_extreme_shapes_train_gpu.py holds the other row kernels to)."""
import pytest
import torch

import embed_positions_bwd_bounds as PB
import extreme_shapes as XS

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF = torch.bfloat16
_SHARED = {}


def _run(dx, cu, P, off, max_len):
    from esme import _hip_embed_positions_bwd as HP
    dp = torch.full((P, dx.shape[1]), PB.PREFILL, dtype=BF, device=DEV)
    out = HP.embed_positions_bwd(dx, cu, P, off, max_len, d_pos=dp)
    assert out is dp
    return dp


def _case(case):
    """Operands on the device, the float64 reference, the bound and the kernel's result: computed once, shared, never modified."""
    if case[0] not in _SHARED:
        dx, cu, P, off, max_len = PB.make_case(case, device=DEV)
        assert dx.stride(0) > dx.shape[1] and dx.data_ptr() % 16 == 0
        cpu = (dx.cpu(), cu.cpu(), P, off, max_len)
        _SHARED[case[0]] = dict(args=(dx, cu, P, off, max_len), cpu=cpu, ref=PB.reference(*cpu), bound=PB.bound(*cpu)[0],
                                got=_run(dx.contiguous(), cu, P, off, max_len))
    return _SHARED[case[0]]


@pytest.mark.parametrize('case', PB.CASES, ids=[c[0] for c in PB.CASES])
def test_gradient_within_bound(case):
    c = _case(case)
    dx, cu, P, off, max_len = c['args']
    got = c['got']
    assert got.dtype == BF and tuple(got.shape) == (P, dx.shape[1])
    worst = PB.worst(got.cpu(), c['ref'], c['bound'])
    print(f'{case[0]}: worst err / bound {worst:.3f}')
    assert worst <= 1.0
    dead = PB.dead_rows(*c['cpu'][1:])
    assert bool((got.cpu()[dead] == 0).all())                              # rows nothing reaches: exact zeros over the 7.0
    assert torch.equal(_run(dx, cu, P, off, max_len), got)                 # a padded row stride
    assert torch.equal(_run(dx.contiguous(), cu, P, off, max_len), got)    # two runs are bit-equal
    # the kernel's order of operations is the emulation's: the same bits
    assert torch.equal(got.cpu().view(torch.int16), PB.emulate(*c['cpu']).view(torch.int16))


@pytest.mark.parametrize('case', PB.CASES, ids=[c[0] for c in PB.CASES])
def test_a_sequence_reaches_only_its_own_rows(case):
    """Doubling the rows of the (first) longest sequence doubles exactly the table rows it alone reaches (a power of two: the same
    roundings), changes the rows it shares and leaves the bits of the rows it does not reach."""
    c = _case(case)
    dx, cu, P, off, max_len = c['args']
    cul = cu.tolist()
    lens = [b - a for a, b in zip(cul[:-1], cul[1:])]
    b = max(range(len(lens)), key=lambda i: lens[i])
    dx2 = dx.contiguous().clone()
    dx2[cul[b]:cul[b + 1]] *= 2
    got = _run(dx2, cu, P, off, max_len)
    fan = PB.fan_in(*c['cpu'][1:]).to(DEV)
    reached = torch.zeros(P, dtype=torch.bool, device=DEV)
    reached[off:off + min(lens[b], max_len)] = True
    alone, shared = reached & (fan == 1), reached & (fan > 1)
    assert torch.equal(got[alone], c['got'][alone] * 2) and torch.equal(got[~reached], c['got'][~reached])
    assert bool(reached.any()) and bool((got[reached] != c['got'][reached]).any(dim=1).all())
    name = case[0].split('-')[0]
    assert bool(alone.any()) == (name in ('one', 'empties', 'mixed')) and bool(shared.any()) == (name != 'one')


def test_nothing_to_sum_writes_zeros():
    from esme import _hip_embed_positions_bwd as HP
    dx = torch.randn(16, 64, device=DEV).to(BF)
    for dxx, cu in ((dx, torch.zeros(1, dtype=torch.int32, device=DEV)),                        # B = 0
                    (dx[:0], torch.zeros(1, dtype=torch.int32, device=DEV)),                    # B = 0 and T = 0
                    (dx[:0], torch.zeros(4, dtype=torch.int32, device=DEV)),                    # T = 0: three empty sequences
                    (dx, torch.zeros(4, dtype=torch.int32, device=DEV))):                       # three empty sequences in front of 16 rows
        dp = _run(dxx, cu, 12, 2, 10)
        assert not bool(dp.any()), (dxx.shape, cu.numel())
    assert not bool(_run(dx, torch.tensor([0, 16], dtype=torch.int32, device=DEV), 12, 2, 0).any())      # max_len = 0: no row is summed
    lib = HP._lib()
    dp = torch.full((12, 64), PB.PREFILL, dtype=BF, device=DEV)
    from esme import _hip
    assert lib.esme_hip_embed_positions_bwd(None, 0, None, 0, 0, 64, 12, 2, 10, dp.data_ptr(), _hip._stream()) == 0      # null operands where nothing is read
    assert not bool(dp.any())


def test_refusals():
    from esme import _hip_embed_positions_bwd as HP
    z = lambda *s: torch.zeros(*s, dtype=BF, device=DEV)
    cu = torch.tensor([0, 10, 16], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match=r'code -2.*E % 8'):
        HP.embed_positions_bwd(z(16, 60), cu, 12, 2, 10)
    with pytest.raises(RuntimeError, match=r'code -1.*misaligned'):
        HP.embed_positions_bwd(z(16, 72)[:, 4:68], cu, 12, 2, 10)          # a pointer 8 bytes off
    with pytest.raises(RuntimeError, match=r'code -1.*row stride'):
        HP.embed_positions_bwd(z(16, 68)[:, :64], cu, 12, 2, 10)           # a row stride of 68
    with pytest.raises(RuntimeError, match=r'code -1.*max_len \+ pos_offset > P'):
        HP.embed_positions_bwd(z(16, 64), cu, 11, 2, 10)
    with pytest.raises(RuntimeError, match=r'code -1.*pos_offset < 0'):
        HP.embed_positions_bwd(z(16, 64), cu, 12, -1, 10)
    lib = HP._lib()
    from esme import _hip
    dx, dp = z(16, 64), z(12, 64)
    call = lambda B, T: lib.esme_hip_embed_positions_bwd(dx.data_ptr(), 64, cu.data_ptr(), B, T, 64, 12, 2, 10, dp.data_ptr(), _hip._stream())
    assert call(-1, 16) == -1 and b'B < 0' in lib.esme_hip_last_error()
    assert call(2, -1) == -1 and b'T < 0' in lib.esme_hip_last_error()
    with pytest.raises(ValueError):
        HP.embed_positions_bwd(z(16, 64), cu.view(1, 3), 12, 2, 10)
    with pytest.raises(ValueError):
        HP.embed_positions_bwd(z(16, 64), cu, 12, 2, 10, d_pos=z(13, 64))
    with pytest.raises(TypeError):
        HP.embed_positions_bwd(z(16, 64), cu.long(), 12, 2, 10)
    with pytest.raises(TypeError):
        HP.embed_positions_bwd(z(16, 64).float(), cu, 12, 2, 10)


def test_70002_short_sequences():
    """More sequences than a grid dimension holds (65 535), lengths 0 .. 3: three table rows with a fan-in of about 52 000, 35 000 and
    17 000, walked by every lane of the few workgroups there are."""
    import numpy as np
    E, off = 64, 2
    lengths = np.random.Generator(np.random.PCG64(3)).integers(0, 4, size=70002).tolist()
    assert len(lengths) > XS.GRID_Z and min(lengths) == 0 and max(lengths) == 3 and 0 in lengths[XS.GRID_Z:] and 3 in lengths[XS.GRID_Z:]
    cu = XS.cu_of(lengths)
    T = int(cu[-1])
    dx, _ = PB.make_dx(T, E, 901)
    args = (dx, cu, 3 + off + 3, off, 3)
    got = _run(dx.to(DEV), cu.to(DEV), *args[2:])
    ratio = PB.worst(got.cpu(), PB.reference(*args), PB.bound(*args)[0])
    print(f'embed_positions_bwd B={len(lengths)}: worst err / bound {ratio:.3f}')
    assert ratio <= 1.0
    assert not bool(got[:off].any()) and not bool(got[off + 3:].any()) and bool(got[off:off + 3].any(dim=1).all())
    assert torch.equal(got.cpu().view(torch.int16), PB.emulate(*args).view(torch.int16))


ROWS_M, ROWS_LD = 70000, 32768          # tests/test_extreme_shapes_train_gpu.py's buffer: row 65 536 starts at element 2^31


def test_row_offsets_past_2_31():
    """d_x as a column block of a (70 000, 32 768) buffer: the rows of the last two sequences start past element 2^31."""
    E, off = 64, 2
    lengths = [30000, 20000, 17000, 2990]
    cu = XS.cu_of(lengths)
    assert int(cu[3]) > 65536 and int(cu[2]) < 65536 < int(cu[3]) and int(cu[-1]) < ROWS_M                  # crossed inside sequence 2 and before sequence 3
    max_len, P = max(lengths), max(lengths) + off + 6
    buf = XS.wide_buffer(ROWS_M, ROWS_LD, BF, DEV)
    try:
        dx = buf[:, 64:64 + E]
        dx.copy_(torch.randn(ROWS_M, E, generator=torch.Generator().manual_seed(902)).to(BF))
        cud = cu.to(DEV)
        got = _run(dx, cud, P, off, max_len)
        plain = _run(dx.contiguous(), cud, P, off, max_len)
        XS.assert_rows_equal(got, plain, 'embed_positions_bwd, row stride 32 768, against a contiguous d_x')
        XS.assert_inside(got, PB.reference(dx, cud, P, off, max_len), PB.bound(dx, cud, P, off, max_len)[0],
                         f'embed_positions_bwd T={ROWS_M}, row stride {ROWS_LD}')
        assert bool(got[off:off + max_len].any(dim=1).all()) and not bool(got[off + max_len:].any())
    finally:
        del buf
        torch.cuda.empty_cache()
