"""The position-table gradient without a GPU: the error bound of tests/embed_positions_bwd_bounds.py accepts a float32 emulation of the
kernel and rejects every defect the emulation can switch on, on the cases tests/test_embed_positions_bwd_gpu.py runs; the host-side
argument checks of the entry point through the cross-compiled library; the bookkeeping of the new header (footprint coverage, binding
table, exported symbols, Makefile); and, on CPU models, mark_trainable(positions=...) and extend_positions."""
import ctypes
import os
import re

import pytest
import torch

import embed_positions_bwd_bounds as PB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'esme_hip_embed_positions_bwd.h')
NAME = 'embed_positions.weight'
_SHARED = {}


def _case(case):
    """Operands, the float64 reference and the bound: computed once per case, shared, never modified."""
    if case[0] not in _SHARED:
        args = PB.make_case(case)
        _SHARED[case[0]] = dict(args=args, ref=PB.reference(*args), bound=PB.bound(*args)[0], dead=PB.dead_rows(*args[1:]))
    return _SHARED[case[0]]


@pytest.mark.parametrize('case', PB.CASES, ids=[c[0] for c in PB.CASES])
def test_bound_accepts_the_faithful_emulation(case):
    c = _case(case)
    got = PB.emulate(*c['args'])
    worst = PB.worst(got, c['ref'], c['bound'])
    print(f'{case[0]}: faithful emulation: worst err / bound {worst:.3f}')
    assert worst <= 1.0
    dead = c['dead']
    assert bool(dead[:c['args'][3]].all()) and bool(dead[c['args'][3] + c['args'][4]:].all())
    assert bool(dead.any()) or case[0].endswith('offset0')                       # (pos_offset = 0 and P = max_len: every row is reached)
    assert bool((got[dead] == 0).all()) and bool((c['bound'][dead] < 1e-30).all())                                   # dead rows: exact zeros
    live = ~dead
    assert bool(live.any()) and float(c['ref'][live].abs().max()) >= 20 * float(c['bound'][live].max())              # the bound resolves the signal


DEFECT_CASES = [(d, c) for d in PB.DEFECTS for c in PB.CASES if PB.defect_applies(d, c)]


@pytest.mark.parametrize('defect,case', DEFECT_CASES, ids=[f'{d}-{c[0]}' for d, c in DEFECT_CASES])
def test_bound_rejects_every_defect(defect, case):
    c = _case(case)
    got = PB.emulate(*c['args'], defect)
    worst = PB.worst(got, c['ref'], c['bound'])
    zero_rows = bool((got[c['dead']] == 0).all())
    print(f'{case[0]} {defect}: worst err / bound {worst:.1f}, dead rows zero: {zero_rows}')
    assert worst > 1.0 or not zero_rows, f'the bound accepts the defect {defect!r}'


def test_every_defect_applies_and_the_cases_cover_the_issue():
    where = {d: [c[0] for dd, c in DEFECT_CASES if dd == d] for d in PB.DEFECTS}
    assert len(PB.DEFECTS) >= 6
    for d in PB.DEFECTS:
        assert where[d], d
    names = [c[0] for c in PB.CASES]
    assert len(names) == len(set(names))
    assert set(where['offset_plus_one']) == set(names) == set(where['drop_last'])
    assert {n for n in names if 'fan300' in n or 'b65' in n} <= set(where['bf16_acc'])
    assert {n for n in names if 'P+38' in n} <= set(where['past_max_len_unwritten'])
    assert {c[1] for c in PB.GRID} == {64, 320} and {c[3] for c in PB.GRID} == {0, 38} and {c[4] for c in PB.GRID} == {2}
    assert {c[2] for c in PB.GRID} == {(5,), (1, 1, 1), (0, 7, 0, 3), (33, 1, 64, 2, 65), tuple(1 + (7 * b) % 70 for b in range(65)), (3,) * 300}
    assert any(c[4] == 0 for c in PB.CASES)                                      # one case with pos_offset = 0
    E, cu, T, P, off, max_len = PB.params(PB.GRID[0])
    assert P == max_len + 2 and T == cu[-1] + PB.TAIL
    assert int(PB.fan_in(torch.tensor(PB.params(PB.GRID[-1])[1]), 5, 2, 3).max()) == 300 and 'fan300' in PB.GRID[-1][0]
    E, cu, T, P, off, max_len = PB.params(PB.EXTRA[1])                          # a sequence longer than max_len gives only its first max_len rows
    assert max_len < max(b - a for a, b in zip(cu[:-1], cu[1:])) and bool(PB.dead_rows(torch.tensor(cu), P, off, max_len)[off + max_len:].all())


# ------------------------------------------------------------------ the header's bookkeeping

def _declared(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r'\b(esme_hip_\w+)\s*\(([^;{}]*?)\)\s*;', text)}


def test_every_pointer_entry_point_has_a_footprint_case():
    import test_embed_positions_bwd_footprint_gpu as G
    names = [n for n, args in _declared().items() if '*' in args]
    assert names == ['esme_hip_embed_positions_bwd']
    covered = {s for c in G.CASES for s in c.symbols}
    for n in names:
        assert n in covered, f'{n}: declared in esme_hip_embed_positions_bwd.h with a pointer argument, but no case in tests/test_embed_positions_bwd_footprint_gpu.py names it'
        assert re.search(rf'\b{n}\b', G.__doc__), f'{n}: missing from the docstring of tests/test_embed_positions_bwd_footprint_gpu.py'
    assert covered <= set(_declared()), covered - set(_declared())
    ids = [c.id for c in G.CASES]
    assert len(ids) == len(set(ids)) == 12
    assert any('E64' in i for i in ids) and any('E320' in i for i in ids) and len({i.split('-')[1] for i in ids}) == 3


def test_header_symbols_exported_and_bound():
    from esme import _hip, _hip_embed_bwd, _hip_embed_positions_bwd as HP, _hip_segment_mean_bwd
    declared = set(_declared())
    assert declared == set(HP.SIGNATURES) == {'esme_hip_embed_positions_bwd'}
    lib = ctypes.CDLL(_hip.lib_path())
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/esme_hip_embed_positions_bwd.h but not exported'
    for other in (_hip, _hip_embed_bwd, _hip_segment_mean_bwd):                  # the other tables and headers keep their own symbols
        assert not declared & set(other.SIGNATURES), other.__name__
    for other in os.listdir(os.path.join(ROOT, 'include')):
        if other != 'esme_hip_embed_positions_bwd.h':
            assert not declared & set(_declared(os.path.join(ROOT, 'include', other))), other
    for name, args in _declared().items():                                       # the number of arguments of each declaration equals the binding's
        assert len([a for a in args.split(',') if a.strip()]) == len(HP.SIGNATURES[name][1]), name
    mk = open(os.path.join(ROOT, 'esm-efficient_amd', 'csrc', 'Makefile')).read()
    srcs = re.search(r'^SRCS\s*:=(.*)$', mk, flags=re.M).group(1)
    hdrs = re.search(r'^HDRS\s*:=(.*)$', mk, flags=re.M).group(1)
    assert 'embed_positions_bwd.hip' in srcs.split() and '../../include/esme_hip_embed_positions_bwd.h' in hdrs.split()


def test_host_validation_of_the_entry_point():
    """Host-side checks need no device: every refusal returns before any launch, with its message."""
    from esme import _hip_embed_positions_bwd as HP
    lib = HP._lib()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    args = dict(dx=p, ld=64, cu=p, B=3, T=30, E=64, P=12, off=2, max_len=10, dp=p, stream=None)
    call = lambda **kw: lib.esme_hip_embed_positions_bwd(*{**args, **kw}.values())
    for bad in (dict(dx=None), dict(cu=None), dict(dp=None),                                    # null pointers
                dict(dx=p + 8), dict(dp=p + 2),                                                  # misaligned
                dict(ld=68), dict(ld=56), dict(ld=0), dict(ld=-64),                              # strides
                dict(B=-1), dict(T=-1), dict(off=-1), dict(max_len=-1), dict(E=0), dict(P=0),    # geometry
                dict(max_len=11), dict(off=3), dict(P=11)):                                      # the table has no row for the last position
        assert call(**bad) == -1, bad
    assert call(dx=p + 8) == -1 and b'misaligned' in lib.esme_hip_last_error()
    assert call(dp=p + 2) == -1 and b'misaligned' in lib.esme_hip_last_error()
    assert call(ld=68) == -1 and b'row stride' in lib.esme_hip_last_error()
    assert call(max_len=11) == -1 and b'max_len + pos_offset > P' in lib.esme_hip_last_error()
    assert call(B=-1) == -1 and b'B < 0' in lib.esme_hip_last_error()
    assert call(off=-1) == -1 and b'pos_offset < 0' in lib.esme_hip_last_error()
    assert call(E=60) == -2 and b'E % 8' in lib.esme_hip_last_error()
    assert call(T=2 ** 31) == -2 and b'2^31' in lib.esme_hip_last_error()
    assert call(B=0, dp=None) == -1 and call(T=0, dp=None) == -1                                 # (nothing to sum still writes d_pos)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        HP.embed_positions_bwd(torch.zeros(4, 64, dtype=torch.bfloat16), torch.tensor([0, 4], dtype=torch.int32), 8, 2, 4)


# ------------------------------------------------------------------ the opt-in on CPU models

def _esm1(tmp_path, kind, seed=5):
    from esme import ESM, synthetic as syn
    path = syn.write_checkpoint(str(tmp_path / f'{kind}.safetensors'), f'{kind}_t', 1, 64, 1, seed=seed)
    return ESM.from_pretrained(path, device='cpu')


@pytest.mark.parametrize('kind', ('esm1b', 'esm1v'))
def test_mark_trainable_positions_truth_table(tmp_path, kind):
    model = _esm1(tmp_path, kind)
    keys = list(model.state_dict())
    w = model.embed_positions.weight
    flags = lambda: {n for n, p in model.named_parameters() if p.requires_grad}
    before = {'emb_layer_norm_before.weight', 'emb_layer_norm_before.bias'} if kind == 'esm1b' else set()
    tok, pad = torch.full((4,), 5, dtype=torch.long), (torch.tensor([0, 4], dtype=torch.int32), 4)
    assert not w.requires_grad and '_train_positions' not in model.__dict__
    base = flags() if model.mark_trainable() is model else None
    assert NAME not in base and before <= base and 'emb_layer_norm_after.weight' in base        # ESM-1b's first LayerNorm trains like the last
    with pytest.raises(NotImplementedError, match='learned-position'):                            # no opt-in: today's refusal
        model.forward_trainable(tok, pad)
    assert model.mark_trainable(positions=True) is model and flags() == base | {NAME} and model.__dict__['_train_positions'] is True
    assert model.mark_trainable(False, False, positions=True) is model and flags() == {NAME}    # the table alone: the reference's experiment
    assert model.mark_trainable(positions='frozen') is model and flags() == base and model.__dict__['_train_positions'] == 'frozen'
    assert model.mark_trainable(False, False, positions='frozen') is model and flags() == set()
    with pytest.raises(RuntimeError, match='no CPU fallback'):                                    # every check passed: the first kernel call says where it must run
        model.forward_trainable(tok, pad)
    model.mark_trainable(positions=True).mark_trainable()                                         # the default withdraws the opt-in and the flag it set
    assert flags() == base and '_train_positions' not in model.__dict__
    with pytest.raises(NotImplementedError, match='learned-position'):
        model.forward_trainable(tok, pad)
    w.requires_grad_(True)                                                                        # a flag set by hand: not touched, and still refused
    model.mark_trainable()
    assert w.requires_grad and '_train_positions' not in model.__dict__
    with pytest.raises(NotImplementedError, match='learned-position'):
        model.forward_trainable(tok, pad)
    w.requires_grad_(False)
    model.mark_trainable(norms=True, layers=[0], positions='frozen')                              # a layer selection leaves the stem's LayerNorm frozen
    assert not before & flags() and 'emb_layer_norm_after.weight' not in flags()
    model.mark_trainable(embedding=True, positions=True)                                          # both tables
    assert {NAME, 'embed_tokens.weight'} <= flags()
    assert list(model.state_dict()) == keys
    model.set_precision('exact')
    with pytest.raises(NotImplementedError, match='precision'):
        model.forward_trainable(tok, pad)
    model.set_precision('fast')
    with pytest.raises(ValueError, match='above maximum'):                                        # the forward's own check, before any launch
        model.forward_trainable(torch.full((5000,), 5, dtype=torch.long), (torch.tensor([0, 5000], dtype=torch.int32), 5000))
    model.quantization = '8bit'
    for qlora in (False, True):
        model._qlora = qlora
        with pytest.raises(NotImplementedError, match='quantised'):
            model.forward_trainable(tok, pad)
    with pytest.raises(NotImplementedError, match='quantised'):
        model.mark_trainable(positions=True)


def test_positions_keyword_is_refused_without_a_position_table(tmp_path):
    from esme import ESM, ESM2, ESMC, synthetic as syn
    for cls in (ESM2, ESMC):
        m = cls(num_layers=1, embed_dim=128, attention_heads=2)
        for value in (True, 'frozen'):
            with pytest.raises(ValueError, match='embed_positions'):
                m.mark_trainable(positions=value)
        assert m.mark_trainable(positions=False) is m and '_train_positions' not in m.__dict__
        with pytest.raises(ValueError, match='embed_positions'):
            m.extend_positions(8192)
    with pytest.raises(ValueError, match="positions"):
        _esm1(tmp_path, 'esm1v').mark_trainable(positions='yes')


@pytest.mark.parametrize('grad', (False, True))
def test_extend_positions(tmp_path, grad):
    from esme.embedding import LearnedPositionalEmbedding
    model = _esm1(tmp_path, 'esm1v')
    if grad:
        model.mark_trainable(False, False, positions=True)
    old = model.embed_positions
    keys = list(model.state_dict())
    table = old.weight.detach().clone()
    assert old.max_positions == 4096 and table.shape[0] == 4098 and bool(table.any())
    assert model.extend_positions(8192) is model
    new = model.embed_positions
    assert isinstance(new, LearnedPositionalEmbedding) and new is not old and new.max_positions == 8192 and new.num_embeddings == 8194
    w = new.weight
    assert w.shape == (8194, 64) and w.dtype == table.dtype and w.device == table.device and w.requires_grad == grad
    assert torch.equal(w.detach()[:4098].view(torch.int16), table.view(torch.int16))            # the old rows bit for bit
    assert not bool(w.detach()[4098:].any())                                                     # the new rows are zeros
    assert list(model.state_dict()) == keys and model.state_dict()[NAME].shape[0] == 8194
    assert model.__dict__.get('_train_positions', False) == (True if grad else False)
    assert model.extend_positions(8192) is model and model.embed_positions.max_positions == 8192 # the same size: nothing to do
    with pytest.raises(ValueError, match='shrink'):
        model.extend_positions(4096)
    assert model.embed_positions.max_positions == 8192


def test_an_extended_table_round_trips_through_a_checkpoint(tmp_path):
    """What tools/position_finetune.py writes: the state dict with esme.synthetic.checkpoint_metadata, read back by ESM.from_pretrained
    with the table at its new size."""
    from safetensors.torch import save_file
    from esme import ESM, synthetic as syn
    model = _esm1(tmp_path, 'esm1b').extend_positions(5000)
    with torch.no_grad():
        model.embed_positions.weight[4500] = 0.25
    path = str(tmp_path / 'extended.safetensors')
    save_file({k: v.detach().contiguous() for k, v in model.state_dict().items()}, path, syn.checkpoint_metadata('esm1b_t', 1, 64, 1))
    again = ESM.from_pretrained(path, device='cpu')
    assert type(again) is type(model) and again.embed_positions.max_positions == 5000 and again.embed_positions.num_embeddings == 5002
    assert list(again.state_dict()) == list(model.state_dict())
    for k, v in model.state_dict().items():
        assert torch.equal(again.state_dict()[k], v), k
    assert not any(p.requires_grad for p in again.parameters())


def test_the_two_forms_of_the_reference_and_the_bound_agree(monkeypatch):
    """Many short sequences are summed position by position (the recurrence of the bound in closed form), few long ones sequence by
    sequence: the same numbers either way, on every case."""
    for case in PB.CASES:
        args = PB.make_case(case)
        forms = []
        for many in (False, True):
            monkeypatch.setattr(PB, '_many', lambda cu_lens, max_len, many=many: many)
            forms.append((PB.reference(*args), *PB.bound(*args)))
        monkeypatch.undo()
        (r0, b0, p0), (r1, b1, p1) = forms
        assert float((r0 - r1).abs().max()) <= 1e-12 * max(1.0, float(r0.abs().max())), case[0]
        assert bool(((p0 - p1).abs() <= 1e-9 * p0.abs()).all()) and bool(((b0 - b1).abs() <= 1e-9 * b0.abs()).all()), case[0]


def test_position_grad_fixture_is_consistent():
    """tests/golden/g18_position_grad.npz (the fixture of tests/test_position_train_gpu.py): numbers only, float64 truths of the right
    shapes, the fan-in of the batch, and bars of the size one bfloat16 pipeline errs by."""
    import numpy as np
    from golden_util import GOLDEN, load_golden
    path = os.path.join(GOLDEN, 'g18_position_grad.npz')
    assert os.path.getsize(path) < 1 << 20
    with np.load(path, allow_pickle=False) as z:
        assert all(z[k].dtype.kind in 'fiub' for k in z.files)
    g, g15 = load_golden('g18_position_grad.npz'), load_golden('g15_full_grad.npz')
    E, ml, cu = int(g['E']), int(g15['max_len']), g15['cu_lens'].long()
    assert int(g['H']) == 2 and E // int(g['H']) == 64                                            # the head dim of the released models
    lens = cu[1:] - cu[:-1]
    for kind in ('esm1b', 'esm1v'):
        truth = g[f'{kind}_oracle/{NAME}']
        assert truth.shape == (ml + 2, E) and truth.dtype == torch.float64
        fan = g[f'{kind}_fan_in'].long()
        assert torch.equal(fan, torch.tensor([0, 0] + [int((lens > p).sum()) for p in range(ml)]))
        assert torch.equal(truth.abs().amax(dim=1) > 0, fan > 0)                                   # a row has a gradient exactly where a sequence reaches it
        names = [NAME, 'embed_tokens.weight', 'layers.0.self_attn.q.weight'] + (['emb_layer_norm_before.weight', 'emb_layer_norm_before.bias'] if kind == 'esm1b' else [])
        for n in names:
            assert 1e-3 < g[f'{kind}_bf16_error/{n}'] < 5e-2 and g[f'{kind}_oracle/{n}'].dtype == torch.float64, n
        assert (f'{kind}_oracle/emb_layer_norm_before.weight' in g) == (kind == 'esm1b')
        assert 3.0 < g[f'{kind}_oracle/loss'] < 6.0
    src = open(os.path.join(GOLDEN, 'make_golden_position_grad.py')).read()
    assert 'import_reference' not in src and 'make_golden as' not in src                          # the oracle only
