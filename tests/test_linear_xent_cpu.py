"""The fused linear + cross-entropy kernel and its Python surface without a GPU: the error bound of tests/linear_xent_bounds.py accepts
a float32 emulation of the stated arithmetic and rejects each of the eight defects the emulation can switch on, on the cases
tests/test_linear_xent_gpu.py runs; the bookkeeping of the new header (binding table, exported symbols, Makefile, footprint coverage);
the host-side argument checks of the entry points through the cross-compiled library; ResidueLabeledDataset, ResidueHead and the
refusals of esme.loss.linear_cross_entropy."""
import ctypes
import os
import re

import pytest
import torch

import linear_xent_bounds as LB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'esme_hip_linear_xent.h')
ARGS = ('x', 'w', 'b', 'y', 'cw', 'g', 'mean')
_SHARED = {}


def _case(case):
    """Operands, the float64 reference and the bound: computed once per case, shared, never modified."""
    if case['name'] not in _SHARED:
        ops = LB.make_case(case)
        args = [ops[k] for k in ARGS]
        _SHARED[case['name']] = dict(ops=ops, args=args, ref=LB.reference(*args), bound=LB.bound(*args))
    return _SHARED[case['name']]


@pytest.mark.parametrize('case', LB.CASES, ids=[c['name'] for c in LB.CASES])
def test_bound_accepts_the_faithful_emulation(case):
    c = _case(case)
    got = LB.emulate(*c['args'])
    worst = LB.worst_of(got, c['ref'], c['bound'])
    print(f"{case['name']}: faithful emulation: worst err / bound " + ' '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    kept = LB._kept(c['ops']['y'], case['C'])
    if case['C'] == 1 or not bool(kept.any()):                                   # one class / nothing kept: exact zeros
        assert float(got['loss']) == 0.0 and not bool(got['dx'].any()) and not bool(got['dw'].any())
    else:                                                                         # the bound resolves the signal
        for name in ('dx', 'dw', 'loss_rows'):
            assert float(c['ref'][name].abs().max()) >= 10 * float(c['bound'][name].max()), name


DEFECT_CASES = [(d, c) for d in LB.DEFECTS for c in LB.CASES if LB.defect_applies(d, c, LB.make_case(c))]


@pytest.mark.parametrize('defect,case', DEFECT_CASES, ids=[f"{d}-{c['name']}" for d, c in DEFECT_CASES])
def test_bound_rejects_every_defect(defect, case):
    c = _case(case)
    got = LB.emulate(*c['args'], defect=defect)
    worst = LB.worst_of(got, c['ref'], c['bound'])
    print(f"{case['name']} {defect}: worst err / bound " + ' '.join(f'{k} {v:.1f}' for k, v in worst.items()))
    assert max(worst.values()) > 1.0, f'the bound accepts the defect {defect!r}'


def test_every_defect_applies_and_the_cases_cover_the_issue():
    where = {d: [c['name'] for dd, c in DEFECT_CASES if dd == d] for d in LB.DEFECTS}
    assert len(LB.DEFECTS) == 8
    for d in LB.DEFECTS:
        assert where[d], d
    names = [c['name'] for c in LB.CASES]
    assert len(names) == len(set(names))
    assert {c['T'] for c in LB.CASES} == {1, 15, 17, 63, 64, 65, 257, 1000}
    assert {c['E'] for c in LB.CASES} == {64, 320, 1280}
    assert {c['C'] for c in LB.CASES} == {1, 2, 3, 16, 17, 33, 64}
    has = lambda **kw: any(all(c[k] == v for k, v in kw.items()) for c in LB.CASES)
    assert has(T=65, C=17, E=320) and has(T=1000, C=33, E=1280)
    assert has(i64=True) and has(i64=False) and has(bias=True) and has(bias=False) and has(cw=True) and has(cw=False)
    assert has(mean=True) and has(mean=False) and has(block=0) and has(block=1) and has(g=3.0)
    assert has(labels='range') and has(labels='none') and has(labels='half')
    for c in LB.CASES:
        if c['labels'] == 'half' and c['T'] >= 15:
            kept = LB._kept(LB.make_case(c)['y'], c['C'])
            assert 0.25 < float(kept.float().mean()) < 0.75 and bool(kept[-1]), c['name']
    ops = LB.make_case(next(c for c in LB.CASES if c['labels'] == 'range'))
    assert {-7, 3, 2 ** 31 - 1} <= set(ops['y'].tolist())


# ------------------------------------------------------------------ the header's bookkeeping

def _declared(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r'\b(esme_hip_\w+)\s*\(([^;{}]*?)\)\s*;', text)}


def test_header_symbols_exported_and_bound():
    from esme import _hip, _hip_embed_bwd, _hip_gemm_wgrad, _hip_linear_xent as HL
    declared = set(_declared())
    assert declared == set(HL.SIGNATURES) == {'esme_hip_linear_xent_fwd_workspace_bytes', 'esme_hip_linear_xent_bwd_workspace_bytes',
                                              'esme_hip_linear_xent_fwd', 'esme_hip_linear_xent_bwd'}
    lib = ctypes.CDLL(_hip.lib_path())
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/esme_hip_linear_xent.h but not exported'
    for other in (_hip, _hip_embed_bwd, _hip_gemm_wgrad):                        # the other tables and headers keep their own symbols
        assert not declared & set(other.SIGNATURES), other.__name__
    for other in os.listdir(os.path.join(ROOT, 'include')):
        if other != 'esme_hip_linear_xent.h':
            assert not declared & set(_declared(os.path.join(ROOT, 'include', other))), other
    for name, args in _declared().items():                                       # the number of arguments of each declaration equals the binding's
        assert len([a for a in args.split(',') if a.strip()]) == len(HL.SIGNATURES[name][1]), name
    mk = open(os.path.join(ROOT, 'esm-efficient_amd', 'csrc', 'Makefile')).read()
    srcs = re.search(r'^SRCS\s*:=(.*)$', mk, flags=re.M).group(1)
    hdrs = re.search(r'^HDRS\s*:=(.*)$', mk, flags=re.M).group(1)
    assert 'linear_xent.hip' in srcs.split() and '../../include/esme_hip_linear_xent.h' in hdrs.split()
    text = open(HEADER).read()
    for macro, value in (('TILE', HL.TILE), ('CHUNK', HL.CHUNK), ('MAX_C', HL.MAX_C)):
        assert re.search(rf'#define ESME_HIP_LINEAR_XENT_{macro} {value}\b', text), macro
    assert (LB.TILE, LB.CHUNK) == (HL.TILE, HL.CHUNK)


def test_every_pointer_entry_point_has_a_footprint_case():
    import test_linear_xent_footprint_gpu as G
    names = [n for n, args in _declared().items() if '*' in args]
    assert names == ['esme_hip_linear_xent_fwd', 'esme_hip_linear_xent_bwd']
    covered = {s for c in G.CASES for s in c.symbols}
    for n in names:
        assert n in covered and re.search(rf'\b{n}\b', G.__doc__), n
    assert covered <= set(_declared()), covered - set(_declared())
    ids = [c.id for c in G.CASES]
    assert len(ids) == len(set(ids)) and any('T65-E320-C17' in i for i in ids)


def test_workspace_queries():
    from esme import _hip_linear_xent as HL
    assert HL.fwd_workspace_bytes(0) == 0 and HL.fwd_workspace_bytes(1) == 8 and HL.fwd_workspace_bytes(65) == 16
    assert HL.bwd_workspace_bytes(0, 64, 3) == 0
    T, E, C = 1000, 320, 17
    tiles, chunks = -(-T // 64), -(-T // 512)
    assert HL.bwd_workspace_bytes(T, E, C) == E * 64 * 2 + C * tiles * 64 * 2 + tiles * 64 * 4 + chunks * C * E * 4      # the header's O(T C + chunks C E)
    lib = HL._lib()
    for args, code, msg in (((-1, 64, 3), -1, b'bad sizes'), ((5, 0, 3), -1, b'bad sizes'), ((5, 12, 3), -2, b'E % 8'),
                            ((5, 64, 0), -2, b'1 <= C <= 64'), ((5, 64, 65), -2, b'1 <= C <= 64'), ((2 ** 31, 64, 3), -2, b'2^31')):
        assert lib.esme_hip_linear_xent_bwd_workspace_bytes(*args) == code and msg in lib.esme_hip_last_error(), args
    assert lib.esme_hip_linear_xent_fwd_workspace_bytes(-1) == -1 and lib.esme_hip_linear_xent_fwd_workspace_bytes(2 ** 31) == -2
    with pytest.raises(RuntimeError, match='E % 8'):
        HL.bwd_workspace_bytes(5, 12, 3)


def test_host_validation_of_the_entry_points():
    """Host-side checks need no device: every refusal returns before any launch, with its code and message."""
    from esme import _hip_linear_xent as HL
    lib = HL._lib()
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    T, E, C = 5, 64, 3
    common = dict(x=p, ld_x=64, w=p, ld_w=64, bias=p, labels=p, i64=1, ignore=-100, cw=p, T=T, E=E, C=C, mean=1)
    fwd = dict(common, loss_rows=p, lse=p, sums=p, ws=p, ws_bytes=HL.fwd_workspace_bytes(T), stream=None)
    bwd = dict(common, lse=p, sums=p, grad=p, want_dx=1, d_x=p, ld_dx=64, want_dw=1, d_w=p, d_b=p, out_f32=0, ws=p,
               ws_bytes=HL.bwd_workspace_bytes(T, E, C), stream=None)
    f = lambda **kw: lib.esme_hip_linear_xent_fwd(*{**fwd, **kw}.values())
    b = lambda **kw: lib.esme_hip_linear_xent_bwd(*{**bwd, **kw}.values())
    err = lib.esme_hip_last_error
    for call in (f, b):
        for bad in (dict(x=None), dict(w=None), dict(labels=None), dict(sums=None), dict(ws=None), dict(lse=None),        # null pointers
                    dict(x=p + 8), dict(w=p + 2), dict(bias=p + 2), dict(cw=p + 4), dict(labels=p + 8), dict(sums=p + 4),  # misaligned
                    dict(lse=p + 4), dict(ws=p + 8),
                    dict(ld_x=68), dict(ld_x=56), dict(ld_w=68), dict(ld_w=0),                                             # strides
                    dict(ws_bytes=fwd['ws_bytes'] - 1 if call is f else bwd['ws_bytes'] - 1),                              # a short workspace
                    dict(T=-1), dict(E=0)):
            assert call(**bad) == -1, bad
        assert call(C=0) == -2 and b'1 <= C <= 64' in err()
        assert call(C=65) == -2 and b'1 <= C <= 64' in err()
        assert call(E=12) == -2 and b'E % 8' in err()
        assert call(T=2 ** 31) == -2 and b'2^31' in err()
        assert call(x=None) == -1 and b'null pointer' in err()
        assert call(x=p + 8) == -1 and b'misaligned' in err()
        assert call(ld_x=68) == -1 and b'row stride' in err()
        assert call(ws_bytes=7) == -1 and b'workspace too small' in err()
    assert f(loss_rows=None) == -1 and f(loss_rows=p + 4) == -1
    for bad in (dict(grad=None), dict(grad=p + 4), dict(d_x=None), dict(d_x=p + 8), dict(ld_dx=68), dict(ld_dx=56), dict(d_w=None),
                dict(d_w=p + 2), dict(d_b=p + 2)):
        assert b(**bad) == -1, bad
    assert b(ld_dx=68) == -1 and b'row stride' in err()
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        HL.linear_xent_fwd(x, torch.zeros(3, 64, dtype=torch.bfloat16), None, torch.zeros(4, dtype=torch.int64))


# ------------------------------------------------------------------ ResidueLabeledDataset

SEQS = ['MKTAYIAKQR', 'ACDEFGHIKLMNPQRSTVWY', 'GG', 'MKV', 'LLLLLLLLLLLLLLL', 'AC', 'WYWYWY']
LABELS = [[i % 3 for i in range(len(s))] for s in SEQS]


def test_residue_dataset_items_align_with_the_tokens():
    from esme.alphabet import tokenize_unpad
    from esme.data import LabeledDataset, ResidueLabeledDataset
    labels = [list(l) for l in LABELS]
    labels[1][4] = -1                                                             # a negative user label is ignored
    ds = ResidueLabeledDataset(SEQS, labels, 30, shuffle=True, random_state=3)
    plain = LabeledDataset(SEQS, [0.0] * len(SEQS), 30, shuffle=True, random_state=3)
    assert ds.sampler == plain.sampler and len(ds) == len(plain) > 1              # the same batches for the same seed
    seen = 0
    for i in range(len(ds)):
        item, batch = ds[i], ds.sampler[i]
        assert set(item) == {'token', 'cu_lens', 'max_len', 'indices', 'label'}
        token, indices, cu, max_len = tokenize_unpad([SEQS[j] for j in batch])
        assert torch.equal(item['token'], token) and torch.equal(item['cu_lens'], cu) and item['max_len'] == max_len
        assert torch.equal(item['indices'], indices) and torch.equal(item['token'], plain[i]['token'])
        lab = item['label']
        assert lab.dtype == torch.int64 and lab.shape == token.shape
        for k, j in enumerate(batch):
            a, e = int(cu[k]), int(cu[k + 1])
            assert e - a == len(SEQS[j]) + 2
            assert int(lab[a]) == -100 and int(lab[e - 1]) == -100                # <cls> and <eos>
            want = [(-100 if v < 0 else v) for v in labels[j]]
            assert lab[a + 1:e - 1].tolist() == want
            seen += 1
    assert seen == len(SEQS)
    item = next(iter(ds.to_dataloader()))
    assert torch.equal(item['label'], ds[0]['label']) and torch.equal(item['token'], ds[0]['token'])


def test_residue_dataset_classes_truncation_and_errors():
    from esme.data import ResidueLabeledDataset
    ss = ['HHEC-X' + 'C' * (len(s) - 6) if len(s) >= 6 else 'HEC'[:len(s)] for s in SEQS]
    ds = ResidueLabeledDataset(SEQS, ss, 1000, shuffle=False, classes='HEC', ignore_index=-1)
    item = ds[0]
    cu = item['cu_lens'].tolist()
    assert item['label'][cu[0]:cu[1]].tolist() == [-1, 0, 0, 1, 2, -1, -1, 2, 2, 2, 2, -1]      # '-' and 'X' are no class
    assert item['label'][cu[2]:cu[3]].tolist() == [-1, 0, 1, -1]
    cut = ResidueLabeledDataset(SEQS, LABELS, 1000, shuffle=False, truncate_len=4)[0]
    lens = (cut['cu_lens'][1:] - cut['cu_lens'][:-1]).tolist()
    assert lens == [min(len(s), 4) + 2 for s in SEQS] and cut['label'].numel() == cut['token'].numel() == sum(lens)
    assert cut['label'][:6].tolist() == [-100, 0, 1, 2, 0, -100]
    with pytest.raises(ValueError, match='sequence 2 has 2 residues but 3 labels'):
        ResidueLabeledDataset(SEQS, LABELS[:2] + [[0, 1, 2]] + LABELS[3:], 100)
    with pytest.raises(ValueError, match='7 sequences but 6'):
        ResidueLabeledDataset(SEQS, LABELS[:6], 100)
    with pytest.raises(ValueError, match='classes'):
        ResidueLabeledDataset(SEQS, LABELS, 100, classes='HEC')
    tensors = ResidueLabeledDataset(SEQS, [torch.tensor(l) for l in LABELS], 1000, shuffle=False)[0]
    assert torch.equal(tensors['label'], ResidueLabeledDataset(SEQS, LABELS, 1000, shuffle=False)[0]['label'])


# ------------------------------------------------------------------ ResidueHead, ResidueModel and the refusals

def test_residue_head_state_dict_and_defaults():
    from esme.head import ResidueHead
    head = ResidueHead(64, 3)
    assert list(head.state_dict()) == ['classifier.weight', 'classifier.bias']
    assert head.classifier.weight.shape == (3, 64) and head.classifier.bias.shape == (3,)
    assert all(p.dtype == torch.bfloat16 and not p.requires_grad for p in head.parameters())
    assert head.requires_grad_(True) is head and all(p.requires_grad for p in head.parameters())
    sd = {'classifier.weight': torch.randn(3, 64), 'classifier.bias': torch.randn(3)}      # a float32 checkpoint of the same names casts on load
    head.load_state_dict(sd)
    assert torch.equal(head.classifier.weight.detach(), sd['classifier.weight'].to(torch.bfloat16))
    assert torch.equal(head.classifier.bias.detach(), sd['classifier.bias'].to(torch.bfloat16))
    for bad in (0, 65):
        with pytest.raises(ValueError, match='num_labels'):
            ResidueHead(64, bad)
    with pytest.raises(ValueError, match='multiple of 8'):
        ResidueHead(60, 3)
    with pytest.raises(TypeError, match='bfloat16'):
        head(torch.zeros(4, 64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):                    # every check passed: the kernel says where it must run
        head.loss(torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(4, dtype=torch.int64))


def test_linear_cross_entropy_refusals():
    from esme.loss import linear_cross_entropy
    from esme.nn import Linear
    from esme.quantization import Linear8bit
    lin, x, y = Linear(64, 3), torch.zeros(2, 4, 64, dtype=torch.bfloat16), torch.zeros(2, 4, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match='x must be bfloat16'):
        linear_cross_entropy(x.float(), lin, y)
    with pytest.raises(NotImplementedError, match='at most 64'):
        linear_cross_entropy(x, Linear(64, 65), y)
    with pytest.raises(NotImplementedError, match='must be bfloat16'):
        linear_cross_entropy(x, Linear(64, 3, dtype=torch.float32), y)
    with pytest.raises(NotImplementedError, match='padded'):
        padded = Linear(64, 3)
        padded.in_features = 60
        linear_cross_entropy(x, padded, y)
    with pytest.raises(NotImplementedError, match='multiple of 8'):
        linear_cross_entropy(torch.zeros(4, 12, dtype=torch.bfloat16), Linear(12, 3), y.reshape(-1)[:4])
    with pytest.raises(ValueError, match='takes 64 features'):
        linear_cross_entropy(torch.zeros(4, 128, dtype=torch.bfloat16), lin, y.reshape(-1)[:4])
    with pytest.raises(ValueError, match='do not match the rows'):
        linear_cross_entropy(x, lin, y.reshape(-1))
    with pytest.raises(TypeError, match='int32 or int64'):
        linear_cross_entropy(x, lin, y.float())
    with pytest.raises(ValueError, match='reduction'):
        linear_cross_entropy(x, lin, y, reduction='none')
    with pytest.raises(ValueError, match=r'weight \(4,\)'):
        linear_cross_entropy(x, lin, y, weight=torch.ones(4))
    q = Linear8bit.__new__(Linear8bit)
    with pytest.raises(NotImplementedError, match='quantised'):
        linear_cross_entropy(x, q, y)


def test_residue_model_checks_the_width():
    from esme import ESM2
    from esme.head import ResidueHead
    from esme.trainer import ResidueModel
    model = ESM2(num_layers=2, embed_dim=64, attention_heads=2)
    rm = ResidueModel(model, ResidueHead(64, 3))
    assert rm.width == 64 and rm.layers is None and not rm.backbone_trains()
    assert ResidueModel(model, ResidueHead(128, 3), layers=[0]).width == 128
    with pytest.raises(ValueError, match='takes 64 features but the representation has 128'):
        ResidueModel(model, ResidueHead(64, 3), layers=[0])
    rm.head.requires_grad_(True)
    groups = rm.param_groups(lr=1e-5, lr_head=1e-3)
    assert len(groups) == 1 and groups[0]['lr'] == 1e-3 and len(groups[0]['params']) == 2
