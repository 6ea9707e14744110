"""GPU tests of the token-embedding gradient (csrc/embed_bwd.hip, include/esme_hip_embed_bwd.h).

The kernel is judged per element against float64, |got - ref64| <= bound with no rms floor (tests/embed_bwd_bounds.py: the bound is the
sum of the kernel's rounding steps and is vetted on the CPU against an emulation with defects, tests/test_embed_bwd_cpu.py), at
T in {1, R - 1, R, R + 1, 2 R + 1, 2 051} x E in {64, 320} x V in {33, 64} (R = 256, the kernel's row chunk) on ids with a proteome-like
skew that hold the `<mask>` id, the `<pad>` id, -1 and V, with mask_idx and pad_idx set; then all rows one id (a fan-in of 2 051), a
tenth of the ids out of range, and mask_idx = pad_idx = -1.  Every case runs on a contiguous dX and on a column view of a wider buffer
(a padded row stride), into a table that held 7.0: the rows of absent and excluded ids must be exact zeros.  Then the bit-exact
properties of the header (run to run, T = 0, independence of the rows' ids from the other rows) and the refusals."""
import pytest
import torch

import embed_bwd_bounds as EB

pytestmark = pytest.mark.gpu
DEV = 'cuda'
_SHARED = {}


def _run(dx, tok, V, m, p):
    from esme import _hip_embed_bwd as HE
    de = torch.full((V, dx.shape[1]), EB.PREFILL, dtype=torch.bfloat16, device=DEV)
    out = HE.embed_bwd(dx, tok, V, m, p, d_table=de)
    assert out is de
    return de


def _case(case):
    """Operands on the device, the float64 reference, the bound and the kernel's result: computed once, shared, never modified."""
    if case[0] not in _SHARED:
        name, T, E, V, kind, m, p = case
        dx, tok = EB.make_case(case, device=DEV)
        assert dx.stride(0) > E and dx.data_ptr() % 16 == 0
        _SHARED[name] = dict(dx=dx, tok=tok, ref=EB.reference(dx, tok, V, m, p), bound=EB.bound(dx, tok, V, m, p)[0],
                             got=_run(dx.contiguous(), tok, V, m, p))
    return _SHARED[case[0]]


@pytest.mark.parametrize('case', EB.CASES, ids=[c[0] for c in EB.CASES])
def test_gradient_within_bound(case):
    name, T, E, V, kind, m, p = case
    c = _case(case)
    got = c['got']
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (V, E)
    worst = EB.worst(got, c['ref'], c['bound'])
    print(f'{name}: worst err / bound {worst:.3f}')
    assert worst <= 1.0
    dead = torch.tensor([v for v in range(V) if v in (m, p) or not bool((c['tok'] == v).any())], device=DEV)
    assert dead.numel() and bool((got[dead] == 0).all())                  # absent and excluded ids: exact zeros over the 7.0
    strided = _run(c['dx'], c['tok'], V, m, p)                              # a padded row stride
    assert torch.equal(strided, got)
    assert torch.equal(_run(c['dx'].contiguous(), c['tok'], V, m, p), got)  # two runs are bit-equal
    # the kernel's order of operations is the emulation's: the same bits
    assert torch.equal(got.cpu(), EB.emulate(c['dx'].cpu(), c['tok'].cpu(), V, m, p))


@pytest.mark.parametrize('V', EB.VS)
def test_no_row_writes_zeros(V):
    from esme import _hip_embed_bwd as HE
    assert HE.workspace_bytes(0, 64, V) == 0
    de = _run(torch.empty(0, 64, dtype=torch.bfloat16, device=DEV), torch.empty(0, dtype=torch.int64, device=DEV), V, 32, 1)
    assert not bool(de.any())


def test_a_row_reaches_only_its_own_table_row():
    """Changing the rows of one id changes the table row of that id alone, bit for bit."""
    case = EB.GRID[-1]
    name, T, E, V, kind, m, p = case
    c = _case(case)
    v = int(torch.bincount(c['tok'][EB._valid(c['tok'], V, m, p)]).argmax())
    dx = c['dx'].contiguous().clone()
    dx[c['tok'] == v] *= 2
    got = _run(dx, c['tok'], V, m, p)
    others = torch.arange(V, device=DEV) != v
    assert torch.equal(got[others], c['got'][others]) and torch.equal(got[v], c['got'][v] * 2)      # (a power of two: the same roundings)


def test_an_exact_size_uninitialised_workspace():
    from esme import _hip_embed_bwd as HE
    case = EB.GRID[-2]
    name, T, E, V, kind, m, p = case
    c = _case(case)
    ws = torch.full((HE.workspace_bytes(T, E, V),), 0xFF, dtype=torch.uint8, device=DEV)
    de = torch.full((V, E), float('nan'), dtype=torch.bfloat16, device=DEV)
    HE.embed_bwd(c['dx'].contiguous(), c['tok'], V, m, p, d_table=de, workspace=ws)
    assert torch.equal(de, c['got'])


def test_refusals():
    from esme import _hip, _hip_embed_bwd as HE
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=DEV)
    tok = torch.zeros(16, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match=r'code -2.*E % 8'):
        HE.embed_bwd(z(16, 60), tok, 33)
    with pytest.raises(RuntimeError, match=r'code -2.*V > 64'):
        HE.embed_bwd(z(16, 64), tok, 65)
    with pytest.raises(RuntimeError, match=r'code -1.*misaligned'):
        HE.embed_bwd(z(16, 72)[:, 4:68], tok, 33)                          # a pointer 8 bytes off
    with pytest.raises(RuntimeError, match=r'code -1.*row stride'):
        HE.embed_bwd(z(16, 68)[:, :64], tok, 33)                           # a row stride of 68
    with pytest.raises(ValueError):
        HE.embed_bwd(z(16, 64), tok[:8], 33)
    with pytest.raises(TypeError):
        HE.embed_bwd(z(16, 64), tok.int(), 33)
    lib = HE._lib()
    dx, de = z(300, 64), z(33, 64)
    tok = torch.zeros(300, dtype=torch.int64, device=DEV)
    need = HE.workspace_bytes(300, 64, 33)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = lib.esme_hip_embed_bwd(dx.data_ptr(), 64, tok.data_ptr(), 300, 64, 33, 32, 1, de.data_ptr(), ws.data_ptr(), need - 1, _hip._stream())
    assert rc == -1 and b'workspace too small' in lib.esme_hip_last_error()
