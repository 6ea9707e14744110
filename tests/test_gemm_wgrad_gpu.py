"""GPU tests of the weight-gradient GEMM (csrc/gemm_wgrad.hip, include/esme_hip_gemm_wgrad.h).

The kernel is judged per element against float64, |got - ref64| <= bound for dW and db with no rms floor (tests/gemm_wgrad_bounds.py:
the bound is the sum of the kernel's rounding steps and is vetted on the CPU against an emulation with defects,
tests/test_gemm_wgrad_cpu.py), at M in {0, 1, 63, 64, 65, 200, 4 099} x (N, K) in {(64, 64), (192, 64), (64, 320), (320, 192)}, with
bf16 and fp32 outputs, with and without db, the operands being column views of wider buffers.  The header's split rule puts every
M <= 256 on the direct path (one chunk, no workspace) and M = 4 099 on the chunked one (17 chunks of 256 rows at each of the four
widths): both paths occur, which test_both_paths_are_covered asserts.  Then the bit-exact properties of the header, one case whose
last row lies more than 2^32 bytes from the base, and the refusals."""
import pytest
import torch

import gemm_wgrad_bounds as WB

pytestmark = pytest.mark.gpu
DEV = 'cuda'
_SHARED = {}
CASES = [(M, nk) for M in WB.MS for nk in WB.NKS]


def _run(dy, x, fmt, bias=True, **kw):
    from esme import _hip_gemm_wgrad as HW
    return HW.gemm_wgrad(dy, x, bias=bias, out_dtype=WB.FMT[fmt], **kw)


def _case(M, nk):
    """Operands on the device, the float64 reference and the bounds: computed once, shared, never modified."""
    if (M, nk) not in _SHARED:
        N, K = nk
        dy, x, by, bx = WB.make_operands(M, N, K, seed=3 + M + N + K, device=DEV)
        assert dy.stride(0) > N and x.stride(0) > K
        _SHARED[M, nk] = dict(dy=dy, x=x, ref=WB.reference_wgrad(dy, x), bound={f: WB.wgrad_bound(dy, x, f) for f in WB.FMT},
                              got={f: _run(dy, x, f) for f in WB.FMT})
    return _SHARED[M, nk]


@pytest.mark.parametrize('fmt', tuple(WB.FMT))
@pytest.mark.parametrize('M,nk', CASES)
def test_gradients_within_bound(M, nk, fmt):
    c = _case(M, nk)
    dW, db = c['got'][fmt]
    assert dW.dtype == WB.FMT[fmt] and tuple(dW.shape) == nk and db.dtype == WB.FMT[fmt] and tuple(db.shape) == nk[:1]
    ww, wb = WB.worst((dW,), c['ref'][:1], c['bound'][fmt][:1]), WB.worst((db,), c['ref'][1:], c['bound'][fmt][1:])
    print(f'M {M} (N, K) {nk} {fmt}: worst err / bound dW {ww:.3f} db {wb:.3f}')
    assert ww <= 1.0 and wb <= 1.0


@pytest.mark.parametrize('fmt', tuple(WB.FMT))
@pytest.mark.parametrize('M,nk', CASES)
def test_without_db_and_run_to_run(M, nk, fmt):
    c = _case(M, nk)
    dW, db = c['got'][fmt]
    dW0, none = _run(c['dy'], c['x'], fmt, bias=False)
    assert none is None and torch.equal(dW0, dW)                         # db = NULL changes no bit of dW
    dW2, db2 = _run(c['dy'], c['x'], fmt)
    assert torch.equal(dW2, dW) and torch.equal(db2, db)                 # two runs are bit-equal
    if M == 0:
        assert not bool(dW.any()) and not bool(db.any())                 # no row: exact zeros


def test_both_paths_are_covered():
    from esme import _hip_gemm_wgrad as HW
    ws = {(M, nk): HW.workspace_bytes(M, *nk) for M, nk in CASES}
    for (M, nk), n in ws.items():
        assert n == WB.workspace_bytes(M, *nk), (M, nk)
    assert any(n == 0 for n in ws.values()) and any(n > 0 for n in ws.values())
    assert all(ws[4099, nk] > 0 for nk in WB.NKS) and all(ws[200, nk] == 0 for nk in WB.NKS)


@pytest.mark.parametrize('fmt', tuple(WB.FMT))
@pytest.mark.parametrize('M', (65, 4099))
def test_zero_dy_gives_exact_zeros(M, fmt):
    c = _case(M, (192, 64))
    dW, db = _run(torch.zeros_like(c['dy']), c['x'], fmt)
    assert not bool(dW.any()) and not bool(db.any())


@pytest.mark.parametrize('fmt', tuple(WB.FMT))
@pytest.mark.parametrize('M', (65, 4099))
def test_permuting_dy_columns_permutes_dw_rows(M, fmt):
    c = _case(M, (320, 192))
    perm = torch.randperm(320, generator=torch.Generator().manual_seed(1)).to(DEV)
    dW, db = c['got'][fmt]
    dWp, dbp = _run(c['dy'][:, perm].contiguous(), c['x'], fmt)
    assert torch.equal(dWp, dW[perm]) and torch.equal(dbp, db[perm])


def test_row_offsets_are_64_bit():
    """M = 70 000 rows of a 64-column view with a row stride of 32 768 elements: the last row lies 4.6e9 bytes from the base."""
    M, N, K, ld = 70000, 64, 64, 32768
    buf = torch.empty(M * ld, dtype=torch.bfloat16, device=DEV).view(M, ld)
    dy = buf[:, 64:64 + N]
    g = torch.Generator().manual_seed(11)
    dy.copy_(torch.randn(M, N, generator=g).to(torch.bfloat16))
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    assert (M - 1) * ld * 2 > 2 ** 32
    ref, bound = WB.reference_wgrad(dy, x), WB.wgrad_bound(dy, x, 'fp32')
    w = WB.worst(_run(dy, x, 'fp32'), ref, bound)
    print(f'64-bit offsets: dy as the strided view, worst err / bound {w:.3f}')
    assert w <= 1.0
    ref, bound = WB.reference_wgrad(x, dy), WB.wgrad_bound(x, dy, 'fp32')
    w = WB.worst(_run(x, dy, 'fp32'), ref, bound)
    print(f'64-bit offsets: x as the strided view, worst err / bound {w:.3f}')
    assert w <= 1.0


def test_refusals():
    from esme import _hip, _hip_gemm_wgrad as HW
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match=r'code -2.*multiples of 64'):
        HW.gemm_wgrad(z(16, 33), z(16, 64))                              # N = 33
    with pytest.raises(RuntimeError, match=r'code -2.*multiples of 64'):
        HW.gemm_wgrad(z(16, 64), z(16, 96))                              # K = 96
    with pytest.raises(RuntimeError, match=r'code -1.*misaligned'):
        HW.gemm_wgrad(z(16, 72)[:, 4:68], z(16, 64))                     # a pointer 8 bytes off
    with pytest.raises(RuntimeError, match=r'code -1.*multiples of 8'):
        HW.gemm_wgrad(z(16, 68)[:, :64], z(16, 64))                      # a row stride of 68
    lib = HW._lib()
    dy, x, dw = z(300, 64), z(300, 64), z(64, 64)
    need = HW.workspace_bytes(300, 64, 64)
    assert need > 0
    rc = lib.esme_hip_gemm_wgrad(dy.data_ptr(), 64, x.data_ptr(), 64, 300, 64, 64, dw.data_ptr(), 64, None, 0, dw.data_ptr(), need - 1, _hip._stream())
    assert rc == -1 and b'workspace too small' in lib.esme_hip_last_error()
