"""The attention backward without a GPU: the error bound of tests/attn_bwd_bounds.py accepts a float32 / bf16 emulation of the kernel and
rejects every defect the emulation can switch on, on the shapes tests/test_attn_bwd_gpu.py runs; the float64 reference against torch's
autograd; the host-side argument checks of the entry point through the cross-compiled library; and the bookkeeping of the new header
(footprint coverage, binding table, exported symbols)."""
import ctypes
import os
import re

import pytest
import torch

import attn_bwd_bounds as AB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'esme_hip_attn_bwd.h')
_SHARED = {}


def _case(d):
    """One batch, a bf16 forward output, the float64 reference and bound: computed once per head dim, shared, never modified."""
    if d not in _SHARED:
        c = AB.make_operands(AB.LENGTHS, AB.HEADS, d, seed=3 + d)
        args = (c['q'], c['k'], c['v'], c['do'], c['cu'], AB.HEADS, d, c['scale'])
        o = AB.forward_bf16(c['q'], c['k'], c['v'], c['cu'], AB.HEADS, d, c['scale'])
        _SHARED[d] = dict(c, o=o, ref=AB.reference_bwd(*args)[:3], bound=AB.bwd_bound(c['q'], c['k'], c['v'], o, *args[3:]))
    return _SHARED[d]


def _emulate(c, d, defect=None):
    return AB.emulate_bwd(c['q'], c['k'], c['v'], c['o'], c['do'], c['cu'], AB.HEADS, d, c['scale'], defect=defect)


def test_reference_equals_autograd():
    c = AB.make_operands((5, 0, 70), 2, 32, seed=2)
    q, k, v = (c[n].double().reshape(-1, 2, 32).requires_grad_() for n in ('q', 'k', 'v'))
    out = []
    for a, b in ((0, 5), (5, 75)):
        s = torch.einsum('ihc,jhc->hij', q[a:b], k[a:b]) * c['scale']
        out.append(torch.einsum('hij,jhc->ihc', torch.softmax(s, 2), v[a:b]))
    o = torch.cat(out)
    o.backward(c['do'].double().reshape(-1, 2, 32))
    ref = AB.reference_bwd(c['q'], c['k'], c['v'], c['do'], c['cu'], 2, 32, c['scale'])
    for g, r in zip((q.grad, k.grad, v.grad, o.detach()), ref):
        assert float((g.reshape(r.shape) - r).abs().max()) < 1e-12


@pytest.mark.parametrize('d', (32, 64))
def test_bound_accepts_the_correct_emulation(d):
    c = _case(d)
    worst = AB.worst(_emulate(c, d), c['ref'], c['bound'])
    print(f'd {d} correct emulation: worst err / bound {worst:.3f}')
    assert worst <= 1.0
    for r, b in zip(c['ref'], c['bound']):                     # the bound resolves the signal: the largest gradient is far above the largest bound
        assert float(r.abs().max()) >= 20 * float(b.max())


@pytest.mark.parametrize('d', (32, 64))
@pytest.mark.parametrize('defect', AB.DEFECTS)
def test_bound_rejects_every_defect(defect, d):
    c = _case(d)
    worst = AB.worst(_emulate(c, d, defect), c['ref'], c['bound'])
    print(f'd {d} {defect}: worst err / bound {worst:.1f}')
    assert worst > 1.0, f'the bound accepts the defect {defect!r}'


def test_single_row_sequence_has_zero_score_gradients():
    """S = 1: P = 1 and dP = D, so dq = dk = 0 and dv = dO, in the reference and in the emulation."""
    c = AB.make_operands((1,), 2, 32, seed=4)
    o = AB.forward_bf16(c['q'], c['k'], c['v'], c['cu'], 2, 32, c['scale'])
    assert torch.equal(o, c['v'])
    dq, dk, dv = AB.emulate_bwd(c['q'], c['k'], c['v'], o, c['do'], c['cu'], 2, 32, c['scale'])
    assert not dq.any() and not dk.any() and torch.equal(dv, c['do'])


# ------------------------------------------------------------------ the header's bookkeeping

def _declared():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r'\b(esme_hip_\w+)\s*\(([^;{}]*?)\)\s*;', text)}


def test_every_pointer_entry_point_has_a_footprint_case():
    import test_attn_bwd_footprint_gpu as G
    names = [n for n, args in _declared().items() if '*' in args]
    assert names == ['esme_hip_attn_varlen_bwd']
    covered = {s for c in G.CASES for s in c.symbols}
    for n in names:
        assert n in covered, f'{n}: declared in esme_hip_attn_bwd.h with a pointer argument, but no case in tests/test_attn_bwd_footprint_gpu.py names it'
        assert re.search(rf'\b{n}\b', G.__doc__), f'{n}: missing from the docstring of tests/test_attn_bwd_footprint_gpu.py'
    assert covered <= set(_declared()), covered - set(_declared())
    ids = [c.id for c in G.CASES]
    assert len(ids) == len(set(ids))


def test_header_symbols_exported_and_bound():
    from esme import _hip, _hip_attn_bwd
    declared = set(_declared())
    assert declared == set(_hip_attn_bwd.SIGNATURES) == {'esme_hip_attn_varlen_bwd_workspace_bytes', 'esme_hip_attn_varlen_bwd'}
    lib = ctypes.CDLL(_hip.lib_path())
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/esme_hip_attn_bwd.h but not exported'
    assert not declared & set(_hip.SIGNATURES)                                   # the main table and header keep their own symbols
    assert 'esme_hip_attn_varlen_bwd' not in open(os.path.join(ROOT, 'include', 'esme_hip.h')).read()
    for name, args in _declared().items():                                       # the number of arguments of each declaration equals the binding's
        assert len([a for a in args.split(',') if a.strip()]) == len(_hip_attn_bwd.SIGNATURES[name][1]), name
    mk = open(os.path.join(ROOT, 'esm-efficient_amd', 'csrc', 'Makefile')).read()
    assert 'attn_bwd.hip' in mk and 'esme_hip_attn_bwd.h' in mk


def test_host_validation_of_the_entry_point():
    """Host-side checks need no device: the size query's stated formula, and the argument errors that return before any launch."""
    from esme import _hip_attn_bwd as HB
    assert HB.workspace_bytes(7, 1000, 20) == 3 * 20 * 1000 * 4
    assert HB.workspace_bytes(0, 0, 1) == 0
    with pytest.raises(RuntimeError, match='bad sizes'):
        HB.workspace_bytes(1, 10, 0)
    lib = HB._lib()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    args = dict(q=p, k=p, v=p, ld=192, o=p, ldo=64, do=p, lddo=64, cu=p, B=1, T=8, H=2, d=32, max_len=8, scale=0.1, dq=p, dk=p, dv=p, ldg=192,
                ws=p, nb=1 << 20, stream=None)
    call = lambda **kw: lib.esme_hip_attn_varlen_bwd(*{**args, **kw}.values())
    for d in (16, 128, 48):
        assert call(d=d, H=1, ldo=192, lddo=192) == -2 and b'head dim must be 32 or 64' in lib.esme_hip_last_error()
    for bad in (dict(ld=60), dict(ldo=56), dict(lddo=68), dict(ldg=32), dict(q=p + 2), dict(o=p + 8), dict(dv=p + 4), dict(ws=p + 4), dict(nb=8),
                dict(k=None), dict(do=None), dict(dq=None), dict(cu=None), dict(ws=None), dict(H=0), dict(T=-1), dict(max_len=0), dict(H=65536, ld=1 << 22, ldo=1 << 22, lddo=1 << 22, ldg=1 << 22),
                dict(T=1 << 31)):
        assert call(**bad) == -1, bad
    assert call(max_len=1 << 27, ld=64) == -2 and b'ESME_HIP_ATTN_BWD_MAX_SEQ_ELEMS' in lib.esme_hip_last_error()
    assert call(max_len=1 << 27, lddo=64, ldo=64, ld=64, ldg=64, d=32) == -2
    assert call(max_len=1 << 26, ldo=128) == -2
    assert call(B=0) == 0 and call(T=0) == 0                                     # nothing to do: no launch
