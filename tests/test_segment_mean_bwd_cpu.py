"""The backward of the per-sequence mean without a GPU: the bit comparison of tests/segment_mean_bwd_bounds.py accepts a CPU emulation
of the kernel and rejects every defect the emulation can switch on, on the cases tests/test_segment_mean_bwd_gpu.py runs; the
host-side argument checks of the entry point through the cross-compiled library; and the bookkeeping of the new header (footprint
coverage, binding table, exported symbols, Makefile)."""
import ctypes
import os
import re

import pytest
import torch

import segment_mean_bwd_bounds as SB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'esme_hip_segment_mean_bwd.h')
_SHARED = {}


def _case(case):
    """Operands and the expected result: computed once per case, shared, never modified."""
    if case[0] not in _SHARED:
        dy, cu, T = SB.make_case(case)
        _SHARED[case[0]] = dict(dy=dy, cu=cu, T=T, want=SB.expected(dy, cu, T))
    return _SHARED[case[0]]


@pytest.mark.parametrize('case', SB.CASES, ids=[c[0] for c in SB.CASES])
def test_bit_equality_accepts_the_faithful_emulation(case):
    c = _case(case)
    got = SB.emulate(c['dy'], c['cu'], c['T'])
    assert SB.equal_bits(got, c['want'])
    cu = c['cu'].tolist()
    assert c['T'] == cu[-1] + SB.TAIL and cu[0] == SB.START
    assert bool((got[:SB.START] == 0).all()) and bool((got[cu[-1]:] == 0).all()) and bool(torch.isfinite(got.float()).all())
    assert bool((got[cu[0]:cu[-1]] != 0).any(dim=1).all())                      # every row of a sequence carries a gradient


DEFECT_CASES = [(d, c) for d in SB.DEFECTS for c in SB.CASES if SB.defect_applies(d, c[1])]


@pytest.mark.parametrize('defect,case', DEFECT_CASES, ids=[f'{d}-{c[0]}' for d, c in DEFECT_CASES])
def test_bit_equality_rejects_every_defect(defect, case):
    c = _case(case)
    assert not SB.equal_bits(SB.emulate(c['dy'], c['cu'], c['T'], defect), c['want']), f'the comparison accepts the defect {defect!r}'


def test_the_cases_cover_the_issue():
    assert SB.LENGTHS == (0, 1, 2, 63, 64, 65, 129, 0, 200) and SB.ES == (8, 64, 1288) and SB.START == 3 and SB.TAIL == 5
    assert {c[1] for c in SB.CASES} == {torch.bfloat16, torch.float32} and len(SB.CASES) == 6
    for d in SB.DEFECTS:
        assert any(dd == d for dd, _ in DEFECT_CASES), d
    # the quotients do round: the definition is not satisfied by an exact division alone
    c = _case(SB.CASES[1])
    lens = (c['cu'][1:] - c['cu'][:-1]).clamp(min=1).double().view(-1, 1)
    assert bool(((c['dy'].double() / lens).to(torch.bfloat16).double() != c['dy'].double() / lens).any())
    # B = 0: zeros
    assert SB.equal_bits(SB.emulate(torch.zeros(0, 8), torch.tensor([4], dtype=torch.int32), 9), torch.zeros(9, 8))
    assert SB.equal_bits(SB.expected(torch.zeros(0, 8), torch.tensor([4], dtype=torch.int32), 9), torch.zeros(9, 8))


# ------------------------------------------------------------------ the header's bookkeeping

def _declared():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r'\b(esme_hip_\w+)\s*\(([^;{}]*?)\)\s*;', text)}


def test_every_pointer_entry_point_has_a_footprint_case():
    import test_segment_mean_bwd_footprint_gpu as G
    names = [n for n, args in _declared().items() if '*' in args]
    assert names == ['esme_hip_segment_mean_bwd']
    covered = {s for c in G.CASES for s in c.symbols}
    for n in names:
        assert n in covered, f'{n}: declared with a pointer argument, but no case in tests/test_segment_mean_bwd_footprint_gpu.py names it'
        assert re.search(rf'\b{n}\b', G.__doc__), f'{n}: missing from the docstring of tests/test_segment_mean_bwd_footprint_gpu.py'
    assert covered <= set(_declared()), covered - set(_declared())
    ids = [c.id for c in G.CASES]
    assert len(ids) == len(set(ids)) and any('float32' in i for i in ids) and any('bfloat16' in i for i in ids)


def test_header_symbols_exported_and_bound():
    from esme import _hip, _hip_segment_mean_bwd as HS
    declared = set(_declared())
    assert declared == set(HS.SIGNATURES) == {'esme_hip_segment_mean_bwd'}
    lib = ctypes.CDLL(_hip.lib_path())
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/esme_hip_segment_mean_bwd.h but not exported'
    assert not declared & set(_hip.SIGNATURES)                                   # the main table and header keep their own symbols
    assert 'esme_hip_segment_mean_bwd' not in open(os.path.join(ROOT, 'include', 'esme_hip.h')).read()
    for name, args in _declared().items():                                       # the number of arguments of each declaration equals the binding's
        assert len([a for a in args.split(',') if a.strip()]) == len(HS.SIGNATURES[name][1]), name
    mk = open(os.path.join(ROOT, 'esm-efficient_amd', 'csrc', 'Makefile')).read()
    srcs = re.search(r'^SRCS\s*:=(.*)$', mk, flags=re.M).group(1)
    hdrs = re.search(r'^HDRS\s*:=(.*)$', mk, flags=re.M).group(1)
    assert 'segment_mean_bwd.hip' in srcs.split() and '../../include/esme_hip_segment_mean_bwd.h' in hdrs.split()
    assert f'#define ESME_HIP_SEGMENT_MEAN_BWD_ROWS {SB.ROWS}\n' in open(HEADER).read() and HS.ROWS == SB.ROWS


def test_host_validation_of_the_entry_point():
    """The argument errors return before any launch, so they need no device."""
    from esme import _hip_segment_mean_bwd as HS
    lib = HS._lib()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    args = dict(dy=p, ldy=64, cu=p, B=3, T=40, E=64, dx=p, ldx=64, f32=0, stream=None)
    call = lambda **kw: lib.esme_hip_segment_mean_bwd(*{**args, **kw}.values())
    for bad in (dict(dy=None), dict(cu=None), dict(dx=None),                                       # null pointers
                dict(dy=p + 8), dict(dx=p + 2),                                                    # misaligned
                dict(ldy=68), dict(ldy=56), dict(ldx=60), dict(ldx=0), dict(ldx=-64),              # strides (bf16: multiples of 8, >= E)
                dict(f32=1, ldx=66), dict(f32=1, ldy=70),                                          # (fp32: multiples of 4)
                dict(B=-1), dict(T=-1), dict(E=0), dict(E=-8)):                                    # geometry
        assert call(**bad) == -1, bad
    assert call(dx=p + 2) == -1 and b'misaligned' in lib.esme_hip_last_error()
    assert call(ldy=68) == -1 and b'row stride' in lib.esme_hip_last_error()
    assert call(E=60, ldx=64) == -2 and b'E % 8' in lib.esme_hip_last_error()
    assert call(T=2 ** 31) == -2 and b'2^31' in lib.esme_hip_last_error()
    assert call(T=0, dx=None, dy=None, cu=None) == 0                                               # (nothing to write)
    assert call(B=0, dx=None) == -1                                                                # (B = 0 still writes d_x)
    with pytest.raises(TypeError, match='bfloat16 or float32'):
        HS.segment_mean_bwd(torch.zeros(2, 8, dtype=torch.float16), torch.tensor([0, 1, 2], dtype=torch.int32), 2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        HS.segment_mean_bwd(torch.zeros(2, 8), torch.tensor([0, 1, 2], dtype=torch.int32), 2)
