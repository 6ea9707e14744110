"""GPU tests of the backward of the per-sequence mean (csrc/segment_mean_bwd.hip, include/esme_hip_segment_mean_bwd.h).

The kernel is judged by bit-equality with the definition, `(dy.float() / len).to(dtype)` gathered per row and zeros for the rows of
no sequence, computed on the CPU (tests/segment_mean_bwd_bounds.py; the comparison is vetted on the CPU against an emulation with
defects, tests/test_segment_mean_bwd_cpu.py): bfloat16 and float32, the lengths (0, 1, 2, 63, 64, 65, 129, 0, 200), E in
(8, 64, 1288), cu_lens[0] = 3 and five rows after the last sequence, into a buffer that held NaN.  Every case also runs into a
strided d_x and from a strided d_y.  Then B = 0, more sequences than a grid dimension holds, the argument errors by code, and what
the kernel is for: esme.autograd.SegmentMean's backward computes the bits of the torch ops it replaces and completes under
torch.cuda.set_sync_debug_mode('error'), which the torch ops did not."""
import pytest
import torch

import segment_mean_bwd_bounds as SB

pytestmark = pytest.mark.gpu
DEV = 'cuda'
_SHARED = {}


def _run(dy, cu, T, ld=None):
    from esme import _hip_segment_mean_bwd as HS
    E = dy.shape[1]
    buf = torch.full((T, ld or E), float('nan'), dtype=dy.dtype, device=DEV)
    dx = buf[:, :E]
    out = HS.segment_mean_bwd(dy, cu, T, d_x=dx)
    assert out is dx
    if ld:
        assert bool(torch.isnan(buf[:, E:]).all())                         # the pad columns of a strided d_x are not written
    return dx


def _case(case):
    """Operands on the device, the expected result (CPU) and the kernel's: computed once, shared, never modified."""
    if case[0] not in _SHARED:
        dy, cu, T = SB.make_case(case, device=DEV)
        _SHARED[case[0]] = dict(dy=dy, cu=cu, T=T, want=SB.expected(dy, cu, T), got=_run(dy, cu, T))
    return _SHARED[case[0]]


@pytest.mark.parametrize('case', SB.CASES, ids=[c[0] for c in SB.CASES])
def test_bit_equal_to_the_definition(case):
    name, dtype, E = case
    c = _case(case)
    got, cu = c['got'], c['cu'].tolist()
    assert got.dtype == dtype and tuple(got.shape) == (c['T'], E)
    assert SB.equal_bits(got, c['want'])
    assert bool((got[:SB.START] == 0).all()) and bool((got[cu[-1]:] == 0).all())           # zeros over the NaN, before and after
    vec = 16 // got.element_size()
    assert SB.equal_bits(_run(c['dy'], c['cu'], c['T'], ld=E + 3 * vec).contiguous(), c['want'])    # a strided d_x
    wide = torch.full((c['dy'].shape[0], E + 2 * vec), float('nan'), dtype=dtype, device=DEV)
    wide[:, vec:vec + E] = c['dy']
    assert SB.equal_bits(_run(wide[:, vec:vec + E], c['cu'], c['T']), c['want'])           # a strided d_y at a column offset
    assert SB.equal_bits(got, SB.emulate(c['dy'], c['cu'], c['T']))                        # the emulation's bits


@pytest.mark.parametrize('dtype', SB.DTYPES, ids=('bfloat16', 'float32'))
def test_no_sequence_writes_zeros(dtype):
    dy, cu = torch.zeros(0, 64, dtype=dtype, device=DEV), torch.tensor([4], dtype=torch.int32, device=DEV)
    got = _run(dy, cu, 70)
    assert SB.equal_bits(got, torch.zeros(70, 64, dtype=dtype))
    from esme import _hip_segment_mean_bwd as HS
    assert HS.segment_mean_bwd(dy, cu, 0).shape == (0, 64)


def test_more_sequences_than_a_grid_dimension():
    """70 000 sequences of one or two rows and a few empty ones: B is no grid dimension of the launch."""
    g = torch.Generator().manual_seed(5)
    lengths = torch.randint(0, 3, (70_000,), generator=g).tolist()
    case = ('many', torch.bfloat16, 8)
    dy, cu, T = SB.make_case(case, device=DEV, lengths=lengths)
    assert dy.shape[0] > 65_535
    assert SB.equal_bits(_run(dy, cu, T), SB.expected(dy, cu, T))


def test_argument_errors_by_code():
    from esme import _hip_segment_mean_bwd as HS
    dy, cu, T = SB.make_case(SB.CASES[1], device=DEV)
    lib, st = HS._lib(), torch.cuda.current_stream().cuda_stream
    dx = torch.full((T, 64), float('nan'), dtype=torch.bfloat16, device=DEV)
    B = dy.shape[0]
    ok = dict(dy=dy.data_ptr(), ldy=64, cu=cu.data_ptr(), B=B, T=T, E=64, dx=dx.data_ptr(), ldx=64, f32=0, stream=st)
    call = lambda **kw: lib.esme_hip_segment_mean_bwd(*{**ok, **kw}.values())
    for bad, code in ((dict(dy=None), -1), (dict(cu=None), -1), (dict(dx=None), -1), (dict(dx=dx.data_ptr() + 2), -1), (dict(ldx=60), -1),
                      (dict(ldy=68), -1), (dict(B=-1), -1), (dict(T=-1), -1), (dict(E=0), -1), (dict(E=60), -2), (dict(T=2 ** 31), -2)):
        assert call(**bad) == code, bad
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all())                                      # a refused call wrote nothing
    with pytest.raises(ValueError, match='cu_lens'):
        HS.segment_mean_bwd(dy, cu[:-1], T)
    with pytest.raises(ValueError, match='d_x'):
        HS.segment_mean_bwd(dy, cu, T, d_x=dx[:-1])
    assert call() == 0
    assert SB.equal_bits(dx, SB.expected(dy, cu, T))


def _torch_backward(dy, cu_lens, rows):
    """SegmentMean.backward as it was in torch ops (two host synchronisations): the bits the kernel must reproduce."""
    lens = (cu_lens[1:] - cu_lens[:-1]).to(torch.long)
    g = (dy.float() / lens.clamp(min=1).view(-1, 1)).to(dy.dtype)
    dx = torch.zeros(rows, dy.shape[1], dtype=dy.dtype, device=dy.device)
    seg = torch.repeat_interleave(torch.arange(lens.numel(), device=dy.device), lens)
    start = int(cu_lens[0])
    dx[start:start + seg.numel()] = g[seg]
    return dx


@pytest.mark.parametrize('case', SB.CASES, ids=[c[0] for c in SB.CASES])
def test_autograd_node_reproduces_the_torch_backward(case):
    from esme.autograd import SegmentMean
    c = _case(case)
    x = torch.randn(c['T'], case[2], device=DEV).to(case[1]).requires_grad_()
    y = SegmentMean.apply(x, c['cu'])
    y.backward(c['dy'])
    assert SB.equal_bits(x.grad, _torch_backward(c['dy'], c['cu'], c['T']))


def test_backward_does_not_synchronise_with_the_host(monkeypatch):
    """The test that fails without the kernel: the torch backward read cu_lens[0] on the host and called repeat_interleave with
    tensor repeats, each a synchronisation, which torch's sync debug mode turns into an error."""
    from esme import _hip
    from esme.autograd import SegmentMean
    c = _case(SB.CASES[1])
    x = torch.randn(c['T'], 64, device=DEV).to(torch.bfloat16).requires_grad_()
    y = SegmentMean.apply(x, c['cu'])
    dy = c['dy'].clone()
    monkeypatch.setattr(_hip, 'TRACE', [])
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        y.backward(dy)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert [t[0] for t in _hip.TRACE] == ['segment_mean_bwd']               # exactly one launch
    monkeypatch.undo()
    assert SB.equal_bits(x.grad, c['want'])
    # the mode is implemented by this build: it does flag a host read
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            int(c['cu'][0])
    finally:
        torch.cuda.set_sync_debug_mode(before)
