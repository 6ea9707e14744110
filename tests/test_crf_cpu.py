"""The linear-chain CRF kernels and their Python surface without a GPU: the float64 dynamic programme of tests/crf_bounds.py against
brute-force enumeration; its error bound accepts a float32 emulation of the stated arithmetic and rejects each of the ten defects the
emulation can switch on, on the cases tests/test_crf_gpu.py runs; the bookkeeping of the new header (binding table, exported symbols,
Makefile, footprint coverage); the host-side argument checks of the entry points through the cross-compiled library; esme.crf.CRF's
state dict and default chain; ResidueCRFHead."""
import ctypes
import os
import re

import pytest
import torch

import crf_bounds as CB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'esme_hip_crf.h')
ARGS = ('e', 'A', 'start', 'end', 'cu', 'tags', 'g')
_SHARED = {}


def _case(case):
    """Operands and the float64 reference with its bound: computed once per case, shared, never modified."""
    if case['name'] not in _SHARED:
        ops = CB.make_case(case)
        args = [ops[k] for k in ARGS]
        _SHARED[case['name']] = dict(ops=ops, args=args, ref=CB.reference(*args, with_bound=True))
    return _SHARED[case['name']]


# ------------------------------------------------------------------ the reference against enumeration

@pytest.mark.parametrize('C,n', [(1, 1), (1, 4), (2, 1), (2, 2), (2, 6), (3, 3), (3, 5), (3, 6)])
def test_dynamic_programming_equals_brute_force(C, n):
    gen = torch.Generator().manual_seed(10 * C + n)
    for trial, grid in enumerate((False, False, True)):
        T = n + 3                                                                     # a frame and one SKIP row inside
        e, A = torch.randn(T, C, generator=gen).double(), torch.randn(C, C, generator=gen).double()
        start, end = torch.randn(C, generator=gen).double(), torch.randn(C, generator=gen).double()
        if grid:                                                                      # coarse values: ties in the Viterbi recursion
            e, A, start, end = ((t * 2).round() / 2 for t in (e, A, start, end))
        tags = torch.full((T,), CB.SKIP, dtype=torch.int32)
        inner = [1 + k + (1 if k >= n // 2 and n > 1 else 0) for k in range(n)]
        for k, t in enumerate(inner):
            tags[t] = CB.FREE if (trial == 0 or k % 2) else int(torch.randint(0, C, (), generator=gen))
        cu = torch.tensor([0, T], dtype=torch.int32)
        g = torch.tensor([1.75])
        ref = CB.reference(e, A, start, end, cu, tags, g)
        rows = CB.chain_rows(cu, tags, C, 0)
        assert [t for t, _ in rows] == inner
        logz, marg, pair, path, best = CB.brute_force(e, A, start, end, rows)
        assert abs(float(ref['logz'][0] - logz)) <= 1e-12
        assert float((ref['de'][inner] - 1.75 * marg).abs().max()) <= 1e-12
        assert float((ref['dA'] - 1.75 * pair).abs().max()) <= 1e-12
        assert float((ref['dstart'] - 1.75 * marg[0]).abs().max()) <= 1e-12 and float((ref['dend'] - 1.75 * marg[-1]).abs().max()) <= 1e-12
        assert abs(float(ref['score'][0] - best)) <= 1e-12
        assert ref['path'][inner].tolist() == path, (trial, ref['path'].tolist(), path)
        assert bool((ref['path'][[t for t in range(T) if t not in inner]] == -100).all()) and not bool(ref['de'][0].any())


# ------------------------------------------------------------------ the bound against the emulation

@pytest.mark.parametrize('case', CB.CASES, ids=[c['name'] for c in CB.CASES])
def test_bound_accepts_the_faithful_emulation(case):
    c = _case(case)
    got = CB.emulate(*c['args'])
    worst = CB.worst_of(got, c['ref'], case['kind'] == 'grid')
    print(f"{case['name']}: faithful emulation: worst err / bound " + ' '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    if case['C'] > 1 and case['kind'] in ('random', 'grid'):                          # the bound resolves the signal (not at |alpha| ~ 10^4, where fp32's ulp is 2^-10)
        for name in ('de', 'dA'):
            assert float(c['ref'][name].abs().max()) >= 10 * float(c['ref']['bound'][name].max()), name


DEFECT_CASES = [(d, c) for d in CB.DEFECTS for c in CB.CASES if CB.defect_applies(d, c)]


@pytest.mark.parametrize('defect,case', DEFECT_CASES, ids=[f"{d}-{c['name']}" for d, c in DEFECT_CASES])
def test_bound_rejects_every_defect(defect, case):
    c = _case(case)
    got = CB.emulate(*c['args'], defect=defect)
    worst = CB.worst_of(got, c['ref'], case['kind'] == 'grid')
    print(f"{case['name']} {defect}: worst err / bound " + ' '.join(f'{k} {v:.1f}' for k, v in worst.items()))
    assert max(worst.values()) > 1.0, f'the bound accepts the defect {defect!r}'


def test_every_defect_applies_and_the_cases_cover_the_issue():
    assert len(CB.DEFECTS) == 10
    for d in CB.DEFECTS:
        assert [c for dd, c in DEFECT_CASES if dd == d], d
    names = [c['name'] for c in CB.CASES]
    assert len(names) == len(set(names))
    assert {c['C'] for c in CB.CASES} >= {1, 2, 3, 9, 33, 64}
    assert {c['kind'] for c in CB.CASES} == {'random', 'large', 'forbidden', 'grid'}
    assert CB.LENGTHS == (0, 1, 2, 3, 4, 63, 64, 65, 130, 0, 257) and CB.rows_of()[:3] == [0, 3, 4] and CB.rows_of()[9] == 2
    for case in CB.CASES:
        ops = _case(case)['ops']
        cu, tags, C = ops['cu'], ops['tags'], case['C']
        assert len(set(ops['g'].tolist())) == cu.numel() - 1                          # per-sequence gradients differ
        inside = skipped = free = chain = 0
        for b in range(cu.numel() - 1):
            a, z = int(cu[b]), int(cu[b + 1])
            if z > a:
                assert not (-1 <= int(tags[a]) < C) and not (-1 <= int(tags[z - 1]) < C)      # the frame rows are outside the chain
            for t in range(a + 1, z - 1):
                inside += 1
                skipped += not (-1 <= int(tags[t]) < C)
                chain += -1 <= int(tags[t]) < C
                free += int(tags[t]) == -1
        assert 0 < skipped < 0.1 * inside
        if case['tags'] == 'mixed':
            assert 0.1 < free / chain < 0.35
    large = _case(next(c for c in CB.CASES if c['kind'] == 'large'))['ops']
    assert 75 <= float(large['e'].abs().max()) <= 80
    grid = _case(next(c for c in CB.CASES if c['name'] == 'C64-grid'))
    assert bool(((grid['ops']['e'] * 16) == (grid['ops']['e'] * 16).round()).all()) and float(grid['ref']['score'].abs().max()) < 2 ** 10
    forb = _case(next(c for c in CB.CASES if c['kind'] == 'forbidden'))
    assert int((forb['ops']['tags'] == 3).sum()) >= 5 and float(forb['ref']['logz'].min()) < -5000 and bool(torch.isfinite(forb['ref']['logz']).all())


# ------------------------------------------------------------------ the header's bookkeeping

def _declared(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r'\b(esme_hip_\w+)\s*\(([^;{}]*?)\)\s*;', text)}


def test_header_symbols_exported_and_bound():
    from esme import _hip, _hip_crf as HC, _hip_linear_xent
    declared = set(_declared())
    assert declared == set(HC.SIGNATURES) == {'esme_hip_crf_bwd_workspace_bytes', 'esme_hip_crf_decode_workspace_bytes', 'esme_hip_crf_fwd',
                                              'esme_hip_crf_bwd', 'esme_hip_crf_decode'}
    lib = ctypes.CDLL(_hip.lib_path())
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/esme_hip_crf.h but not exported'
    for other in (_hip, _hip_linear_xent):
        assert not declared & set(other.SIGNATURES), other.__name__
    for other in os.listdir(os.path.join(ROOT, 'include')):
        if other != 'esme_hip_crf.h':
            assert not declared & set(_declared(os.path.join(ROOT, 'include', other))), other
    for name, args in _declared().items():
        assert len([a for a in args.split(',') if a.strip()]) == len(HC.SIGNATURES[name][1]), name
    mk = open(os.path.join(ROOT, 'esm-efficient_amd', 'csrc', 'Makefile')).read()
    srcs = re.search(r'^SRCS\s*:=(.*)$', mk, flags=re.M).group(1)
    hdrs = re.search(r'^HDRS\s*:=(.*)$', mk, flags=re.M).group(1)
    assert 'crf.hip' in srcs.split() and '../../include/esme_hip_crf.h' in hdrs.split()
    text = open(HEADER).read()
    for macro, value in (('FREE', HC.FREE), ('SKIP', HC.SKIP), ('MAX_C', HC.MAX_C), ('PARTS', HC.PARTS)):
        assert re.search(rf'#define ESME_HIP_CRF_{macro} {value}\b', text), macro
    assert (CB.FREE, CB.SKIP) == (HC.FREE, HC.SKIP)


def test_every_pointer_entry_point_has_a_footprint_case():
    import test_crf_footprint_gpu as G
    names = [n for n, args in _declared().items() if '*' in args]
    assert names == ['esme_hip_crf_fwd', 'esme_hip_crf_bwd', 'esme_hip_crf_decode']
    covered = {s for c in G.CASES for s in c.symbols}
    for n in names:
        assert n in covered and re.search(rf'\b{n}\b', G.__doc__), n
    assert covered == set(_declared())
    ids = [c.id for c in G.CASES]
    assert len(ids) == len(set(ids))


def test_workspace_queries():
    from esme import _hip_crf as HC
    assert HC.bwd_workspace_bytes(0, 0, 3) == 0 and HC.bwd_workspace_bytes(5, 100, 3) == 5 * 15 * 4
    assert HC.bwd_workspace_bytes(70000, 210000, 64) == 1024 * (64 * 64 + 128) * 4           # a partition that depends on B alone
    assert HC.decode_workspace_bytes(0, 3) == 0 and HC.decode_workspace_bytes(7, 3) == 32 and HC.decode_workspace_bytes(16, 64) == 1024
    lib = HC._lib()
    err = lib.esme_hip_last_error
    for args, code, msg in (((-1, 5, 3), -1, b'bad sizes'), ((5, -1, 3), -1, b'bad sizes'), ((5, 5, 0), -2, b'1 <= C <= 64'),
                            ((5, 5, 65), -2, b'1 <= C <= 64'), ((5, 2 ** 31, 3), -2, b'2^31')):
        assert lib.esme_hip_crf_bwd_workspace_bytes(*args) == code and msg in err(), args
    assert lib.esme_hip_crf_decode_workspace_bytes(-1, 3) == -1 and lib.esme_hip_crf_decode_workspace_bytes(2 ** 31, 3) == -2
    assert lib.esme_hip_crf_decode_workspace_bytes(5, 65) == -2
    with pytest.raises(RuntimeError, match='1 <= C <= 64'):
        HC.bwd_workspace_bytes(5, 5, 65)


def test_host_validation_of_the_entry_points():
    """Host-side checks need no device: every refusal returns before any launch, with its code and message."""
    from esme import _hip_crf as HC
    lib = HC._lib()
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    B, T, C = 2, 7, 3
    common = dict(e=p, ld_e=3, A=p, start=p, end=p, cu=p, tags=p, B=B, T=T, C=C)
    fwd = dict(common, logz=p, alpha=p, stream=None)
    bwd = dict(common, alpha=p, logz=p, grad=p, d_e=p, ld_de=3, want=1, d_A=p, d_s=p, d_n=p, ws=p, ws_bytes=HC.bwd_workspace_bytes(B, T, C), stream=None)
    dec = dict(common, path=p, i64=1, fill=-100, score=p, ws=p, ws_bytes=HC.decode_workspace_bytes(T, C), stream=None)
    f = lambda **kw: lib.esme_hip_crf_fwd(*{**fwd, **kw}.values())
    b = lambda **kw: lib.esme_hip_crf_bwd(*{**bwd, **kw}.values())
    d = lambda **kw: lib.esme_hip_crf_decode(*{**dec, **kw}.values())
    err = lib.esme_hip_last_error
    for call in (f, b, d):
        for bad in (dict(e=None), dict(A=None), dict(start=None), dict(end=None), dict(cu=None), dict(tags=None),      # null pointers
                    dict(e=p + 4), dict(A=p + 8), dict(start=p + 4), dict(end=p + 4), dict(cu=p + 4), dict(tags=p + 8),   # misaligned
                    dict(ld_e=2), dict(ld_e=0), dict(B=-1), dict(T=-1)):
            assert call(**bad) == -1, bad
        assert call(C=0) == -2 and b'1 <= C <= 64' in err()
        assert call(C=65) == -2 and b'1 <= C <= 64' in err()
        assert call(T=2 ** 31) == -2 and b'2^31' in err()
        assert call(e=None) == -1 and b'null pointer' in err()
        assert call(e=p + 4) == -1 and b'misaligned' in err()
        assert call(ld_e=2) == -1 and b'row stride' in err()
        assert call(B=0, **({'want': 0} if call is b else {})) == 0                   # nothing to do (and nothing to launch)
    for bad in (dict(logz=None), dict(logz=p + 4), dict(alpha=None), dict(alpha=p + 8)):
        assert f(**bad) == -1 and b(**bad) == -1, bad
    for bad in (dict(grad=None), dict(grad=p + 4), dict(d_e=None), dict(d_e=p + 4), dict(ld_de=2), dict(d_A=None), dict(d_A=p + 4), dict(d_s=None),
                dict(d_n=p + 8), dict(ws=None), dict(ws=p + 8), dict(ws_bytes=bwd['ws_bytes'] - 1)):
        assert b(**bad) == -1, bad
    assert b(ws_bytes=7) == -1 and b'workspace too small' in err()
    assert b(ld_de=2) == -1 and b'row stride' in err()
    for bad in (dict(path=None), dict(path=p + 8), dict(score=None), dict(score=p + 4), dict(ws=None), dict(ws=p + 4), dict(ws_bytes=dec['ws_bytes'] - 1)):
        assert d(**bad) == -1, bad
    assert d(ws_bytes=7) == -1 and b'workspace too small' in err()
    e = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        HC.crf_fwd(e, torch.zeros(3, 3), torch.zeros(3), torch.zeros(3), torch.tensor([0, 4], dtype=torch.int32), torch.zeros(4, dtype=torch.int32))


# ------------------------------------------------------------------ esme.crf.CRF and ResidueCRFHead

def test_crf_state_dict_and_masks():
    from esme.crf import CRF, FORBIDDEN
    crf = CRF(4)
    assert list(crf.state_dict()) == ['transitions', 'start_transitions', 'end_transitions', 'allowed', 'allowed_start', 'allowed_end']
    assert [n for n, _ in crf.named_parameters()] == ['transitions', 'start_transitions', 'end_transitions']       # pytorch-crf's keys
    assert all(p.dtype == torch.float32 and not p.requires_grad for p in crf.parameters())
    assert crf.transitions.shape == (4, 4) and crf.start_transitions.shape == (4,) and crf.end_transitions.shape == (4,)
    sd = {'transitions': torch.randn(4, 4, dtype=torch.float64), 'start_transitions': torch.randn(4, dtype=torch.float64),
          'end_transitions': torch.randn(4, dtype=torch.float64)}                     # an fp64 dict of pytorch-crf's shape
    crf.load_state_dict(sd, strict=False)
    assert torch.equal(crf.transitions.detach(), sd['transitions'].float()) and crf.transitions.dtype == torch.float32
    assert torch.equal(crf.end_transitions.detach(), sd['end_transitions'].float())
    allowed = torch.ones(4, 4, dtype=torch.bool)
    allowed[0, 2] = False
    masked = CRF(4, allowed=allowed, allowed_start=[True, True, False, True])
    A, s, n = masked.scores()
    assert FORBIDDEN == -10000.0 and float(A[0, 2]) == float(masked.transitions[0, 2] - 10000.0)
    assert float(A[1, 2]) == float(masked.transitions[1, 2]) and float(s[2]) == float(masked.start_transitions[2] - 10000.0)
    assert torch.equal(n, masked.end_transitions)
    assert crf.requires_grad_(True) is crf and all(p.requires_grad for p in crf.parameters())
    for bad in (0, 65):
        with pytest.raises(ValueError, match='num_labels'):
            CRF(bad)
    with pytest.raises(ValueError, match='allowed must have shape'):
        CRF(4, allowed=torch.ones(3, 3, dtype=torch.bool))
    cu = torch.tensor([0, 5], dtype=torch.int32)
    with pytest.raises(ValueError, match='packed'):
        crf.loss(torch.zeros(1, 5, 4), torch.zeros(5, dtype=torch.int64), cu)
    with pytest.raises(ValueError, match='4 labels'):
        crf.decode(torch.zeros(5, 3), cu)
    with pytest.raises(ValueError, match='reduction'):
        crf.loss(torch.zeros(5, 4), torch.zeros(5, dtype=torch.int64), cu, reduction='none')
    with pytest.raises(RuntimeError, match='no CPU fallback'):                        # every check passed: the kernel says where it must run
        crf.loss(torch.zeros(5, 4), torch.zeros(5, dtype=torch.int64), cu)


def test_default_chain_matches_the_residue_dataset():
    from esme.crf import default_chain
    from esme.data import ResidueLabeledDataset
    seqs = ['MKTAYIAKQR', 'GG', 'M', 'ACDEFGHIKLMNPQRSTVWY']
    item = ResidueLabeledDataset(seqs, [[i % 3 for i in range(len(s))] for s in seqs], 1000, shuffle=False)[0]
    chain = default_chain(item['cu_lens'], item['token'].numel())
    assert torch.equal(chain, item['label'] != -100)
    cu = torch.tensor([0, 0, 3, 3, 5, 6, 6], dtype=torch.int32)                       # empty sequences first, inside and last; 1- and 2-row ones
    assert default_chain(cu, 6).tolist() == [False, True, False, False, False, False]
    assert default_chain(torch.tensor([0], dtype=torch.int32), 0).numel() == 0


def test_residue_crf_head_and_model():
    from esme import ESM2
    from esme.head import ResidueCRFHead, ResidueHead
    from esme.trainer import ResidueModel
    head = ResidueCRFHead(64, 3, allowed_end=[True, False, True])
    assert list(head.state_dict()) == ['crf.transitions', 'crf.start_transitions', 'crf.end_transitions', 'crf.allowed', 'crf.allowed_start',
                                       'crf.allowed_end', 'classifier.weight', 'classifier.bias']
    assert head.classifier.weight.dtype == torch.bfloat16 and head.crf.transitions.dtype == torch.float32
    assert not any(p.requires_grad for p in head.parameters())
    head.requires_grad_(True)
    em = head.emissions_trainable(torch.zeros(5, 64, dtype=torch.bfloat16))
    assert em.shape == (5, 3) and em.dtype == torch.float32 and em.grad_fn is not None
    with pytest.raises(TypeError, match='bfloat16'):
        head.emissions_trainable(torch.zeros(5, 64))
    plain = ResidueHead(64, 3)
    plain.load_state_dict({k: v for k, v in head.state_dict().items() if k.startswith('classifier.')})    # the classifier's keys are ResidueHead's
    model = ESM2(num_layers=2, embed_dim=64, attention_heads=2)
    rm = ResidueModel(model, head)
    assert rm.width == 64 and len(rm.param_groups()[0]['params']) == 5
    with pytest.raises(ValueError, match='takes 64 features'):
        ResidueModel(model, ResidueCRFHead(64, 3), layers=[0])
