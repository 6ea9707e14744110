"""The token-embedding gradient and the masked-token datasets without a GPU: the error bound of tests/embed_bwd_bounds.py accepts a
float32 emulation of the kernel and rejects every defect the emulation can switch on, on the cases tests/test_embed_bwd_gpu.py runs;
the host-side argument checks of the entry points through the cross-compiled library; the bookkeeping of the new header (footprint
coverage, binding table, exported symbols, Makefile); the properties of esme.alphabet.mask_tokens, on this package's output and on
the reference's recorded one (tests/golden/g16_mask_tokens.npz); the masked datasets' items; the fixture of tests/test_mlm_train_gpu.py;
and mark_trainable(embedding=...) on a CPU model."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import embed_bwd_bounds as EB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'esme_hip_embed_bwd.h')
FASTA = os.path.join(ROOT, 'tests', 'golden', 'data', 'test.fa')
_SHARED = {}


def _case(case):
    """Operands, the float64 reference and the bound: computed once per case, shared, never modified."""
    if case[0] not in _SHARED:
        name, T, E, V, kind, m, p = case
        dx, tok = EB.make_case(case)
        _SHARED[name] = dict(dx=dx, tok=tok, ref=EB.reference(dx, tok, V, m, p), bound=EB.bound(dx, tok, V, m, p)[0])
    return _SHARED[case[0]]


@pytest.mark.parametrize('case', EB.CASES, ids=[c[0] for c in EB.CASES])
def test_bound_accepts_the_faithful_emulation(case):
    name, T, E, V, kind, m, p = case
    c = _case(case)
    got = EB.emulate(c['dx'], c['tok'], V, m, p)
    worst = EB.worst(got, c['ref'], c['bound'])
    print(f'{name}: faithful emulation: worst err / bound {worst:.3f}')
    assert worst <= 1.0
    dead = torch.tensor([v for v in range(V) if v in (m, p) or not bool((c['tok'] == v).any())])
    assert dead.numel() and bool((got[dead] == 0).all()) and float(c['bound'][dead].max()) < 1e-30      # absent and excluded rows: exact zeros
    if T >= EB.ROWS:                          # the bound resolves the signal
        assert float(c['ref'].abs().max()) >= 20 * float(c['bound'].max())


DEFECT_CASES = [(d, c) for d in EB.DEFECTS for c in EB.CASES if EB.defect_applies(d, EB.make_case(c)[1], c[3], c[5], c[6])]


@pytest.mark.parametrize('defect,case', DEFECT_CASES, ids=[f'{d}-{c[0]}' for d, c in DEFECT_CASES])
def test_bound_rejects_every_defect(defect, case):
    name, T, E, V, kind, m, p = case
    c = _case(case)
    worst = EB.worst(EB.emulate(c['dx'], c['tok'], V, m, p, defect), c['ref'], c['bound'])
    print(f'{name} {defect}: worst err / bound {worst:.1f}')
    assert worst > 1.0, f'the bound accepts the defect {defect!r}'


def test_every_defect_applies_and_the_cases_cover_the_issue():
    where = {d: [c[0] for dd, c in DEFECT_CASES if dd == d] for d in EB.DEFECTS}
    for d in EB.DEFECTS:
        assert where[d], d
    grid = [c[0] for c in EB.GRID]
    for d in ('count_mask', 'count_pad', 'wrap_ids', 'absent_unwritten'):     # everywhere from one full chunk on
        assert set(where[d]) >= {n for n in grid if not n.startswith('T1-')}, d
    assert set(where['id_plus_one']) >= set(grid) and set(where['absent_unwritten']) >= set(grid)
    assert {n for n in grid if not n.startswith(f'T{EB.ROWS}-')} <= set(where['drop_tail'])
    assert 'one-id' in where['bf16_acc']
    tok = EB.make_case(EB.EXTRA[0])[1]
    assert int(torch.bincount(tok).max()) >= 1000                             # the fan-in the bf16-accumulation defect needs
    assert {(T, E, V) for _, T, E, V, *_ in EB.GRID} == {(T, E, V) for T in (1, 255, 256, 257, 513, 2051) for E in (64, 320) for V in (33, 64)}
    tok = EB.make_case(EB.EXTRA[1])[1]
    assert bool((tok == -1).any()) and bool((tok == 33).any())
    assert any(c[5] == -1 and c[6] == -1 for c in EB.CASES) and any(c[5] >= 0 and c[6] >= 0 for c in EB.CASES)
    skew = torch.bincount(EB.make_tokens(50000, 33, 'skew', 1, 32, 1).clamp(0, 32), minlength=33).double() / 50000
    assert 0.15 < float(skew.max()) < 0.4 and float(skew[EB.ABSENT]) == 0 and int((skew < 0.02).sum()) > 16


# ------------------------------------------------------------------ the header's bookkeeping

def _declared():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r'\b(esme_hip_\w+)\s*\(([^;{}]*?)\)\s*;', text)}


def test_every_pointer_entry_point_has_a_footprint_case():
    import test_embed_bwd_footprint_gpu as G
    names = [n for n, args in _declared().items() if '*' in args]
    assert names == ['esme_hip_embed_bwd']
    covered = {s for c in G.CASES for s in c.symbols}
    for n in names:
        assert n in covered, f'{n}: declared in esme_hip_embed_bwd.h with a pointer argument, but no case in tests/test_embed_bwd_footprint_gpu.py names it'
        assert re.search(rf'\b{n}\b', G.__doc__), f'{n}: missing from the docstring of tests/test_embed_bwd_footprint_gpu.py'
    assert covered <= set(_declared()), covered - set(_declared())
    ids = [c.id for c in G.CASES]
    assert len(ids) == len(set(ids))
    assert any('V33' in i for i in ids) and any('V64' in i for i in ids) and any('T513' in i for i in ids) and any('T255' in i for i in ids)


def test_header_symbols_exported_and_bound():
    from esme import _hip, _hip_embed_bwd
    declared = set(_declared())
    assert declared == set(_hip_embed_bwd.SIGNATURES) == {'esme_hip_embed_bwd_workspace_bytes', 'esme_hip_embed_bwd'}
    lib = ctypes.CDLL(_hip.lib_path())
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/esme_hip_embed_bwd.h but not exported'
    assert not declared & set(_hip.SIGNATURES)                                   # the main table and header keep their own symbols
    assert 'esme_hip_embed_bwd' not in open(os.path.join(ROOT, 'include', 'esme_hip.h')).read()
    for name, args in _declared().items():                                       # the number of arguments of each declaration equals the binding's
        assert len([a for a in args.split(',') if a.strip()]) == len(_hip_embed_bwd.SIGNATURES[name][1]), name
    mk = open(os.path.join(ROOT, 'esm-efficient_amd', 'csrc', 'Makefile')).read()
    srcs = re.search(r'^SRCS\s*:=(.*)$', mk, flags=re.M).group(1)
    hdrs = re.search(r'^HDRS\s*:=(.*)$', mk, flags=re.M).group(1)
    assert 'embed_bwd.hip' in srcs.split() and '../../include/esme_hip_embed_bwd.h' in hdrs.split()
    text = open(HEADER).read()
    assert f'#define ESME_HIP_EMBED_BWD_ROWS {EB.ROWS}\n' in text and _hip_embed_bwd.ROWS == EB.ROWS
    assert f'#define ESME_HIP_EMBED_BWD_MAX_V {_hip_embed_bwd.MAX_V}\n' in text


def test_host_validation_of_the_entry_points():
    """Host-side checks need no device: the size query's stated formula and geometry errors, and the argument errors that return
    before any launch."""
    from esme import _hip_embed_bwd as HE
    for T, E, V in [(0, 64, 33), (1, 64, 33), (255, 8, 1), (256, 320, 64), (257, 64, 33), (50000, 1280, 33), (2 ** 31 - 1, 8, 64)]:
        assert HE.workspace_bytes(T, E, V) == -(-T // EB.ROWS) * V * E * 4, (T, E, V)
    assert HE.workspace_bytes(50000, 1280, 33) == 196 * 33 * 1280 * 4
    lib = HE._lib()
    q = lib.esme_hip_embed_bwd_workspace_bytes
    assert q(10, 60, 33) == -2 and b'E % 8' in lib.esme_hip_last_error()
    assert q(10, 64, 65) == -2 and b'V > 64' in lib.esme_hip_last_error()
    assert q(2 ** 31, 64, 33) == -2 and b'2^31' in lib.esme_hip_last_error()
    assert q(-1, 64, 33) == -1 and q(10, 0, 33) == -1 and q(10, 64, 0) == -1 and q(10, -8, 33) == -1
    with pytest.raises(RuntimeError, match='code -2'):
        HE.workspace_bytes(10, 60, 33)
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    need = HE.workspace_bytes(300, 64, 33)
    assert need == 2 * 33 * 64 * 4
    args = dict(dx=p, ld=64, tok=p, T=300, E=64, V=33, mask=32, pad=1, de=p, ws=p, nb=need, stream=None)
    call = lambda **kw: lib.esme_hip_embed_bwd(*{**args, **kw}.values())
    for bad in (dict(dx=None), dict(tok=None), dict(de=None), dict(ws=None),                     # null pointers
                dict(dx=p + 8), dict(de=p + 2), dict(ws=p + 4),                                  # misaligned
                dict(ld=68), dict(ld=56), dict(ld=0), dict(ld=-64),                               # strides
                dict(nb=need - 1), dict(nb=0), dict(T=-1), dict(E=0), dict(V=0), dict(V=-3)):     # workspace, geometry
        assert call(**bad) == -1, bad
    assert call(nb=need - 1) == -1 and b'workspace too small' in lib.esme_hip_last_error()
    assert call(dx=p + 8) == -1 and b'misaligned' in lib.esme_hip_last_error()
    assert call(ld=68) == -1 and b'row stride' in lib.esme_hip_last_error()
    assert call(E=60) == -2 and call(V=65) == -2 and call(T=2 ** 31) == -2
    assert call(T=0, de=None) == -1                                                              # (T = 0 still writes d_table)


# ------------------------------------------------------------------ mask_tokens

def check_mask_properties(tokens, masked, mask, freq, alter, alphabet, sigmas=5.0):
    """The documented behaviour of mask_tokens on one (tokens, masked, mask): shapes, special tokens untouched, a selection in every
    row that has an eligible position, and -- where `freq` / `alter` are given -- the selected share and the three outcome shares within
    `sigmas` binomial standard deviations of their marginals.  Returns the counts."""
    assert masked.shape == tokens.shape == mask.shape and mask.dtype == torch.bool and masked.dtype == tokens.dtype
    special = (tokens == alphabet.cls_idx) | (tokens == alphabet.eos_idx) | (tokens == alphabet.padding_idx)
    assert not bool((mask & special).any()), 'a special token was selected'
    assert torch.equal(masked[~mask], tokens[~mask]), 'a position outside the mask changed'
    rows_m, rows_e = (mask.reshape(1, -1), (~special).reshape(1, -1)) if tokens.ndim == 1 else (mask, ~special)
    assert bool((rows_m.any(dim=1) | ~rows_e.any(dim=1)).all()), 'a row without a selection'
    lo, hi = alphabet.amino_acids_idx[0], alphabet.amino_acids_idx[-1] + 1
    sel_in, sel_out = tokens[mask], masked[mask]
    is_mask, is_orig = sel_out == alphabet.mask_idx, sel_out == sel_in
    is_rand = ~is_mask & ~is_orig
    assert bool(((sel_out[is_rand] >= lo) & (sel_out[is_rand] < hi)).all()), 'a replacement outside the amino-acid ids'
    n_valid, n_sel = int((~special).sum()), int(mask.sum())
    counts = dict(valid=n_valid, selected=n_sel, mask=int(is_mask.sum()), random=int(is_rand.sum()), original=int(is_orig.sum()))
    if freq is not None:
        def within(k, n, p, what):
            sd = math.sqrt(n * p * (1 - p))
            assert abs(k - n * p) <= sigmas * sd + 1, f'{what}: {k} of {n}, expected {n * p:.1f} +- {sd:.1f}'
        A = hi - lo
        in_range = (sel_in >= lo) & (sel_in < hi)                            # (the random id can equal the original only inside the range)
        share = float(in_range.double().mean()) if n_sel else 0.0
        p_orig = alter + alter * (1 - alter) * share / A
        within(n_sel, n_valid, freq, 'selected')                             # (the forced selections of empty rows: at most one per row, rare)
        within(counts['mask'], n_sel, (1 - alter) ** 2, '<mask>')
        within(counts['random'], n_sel, alter * (1 - alter) - alter * (1 - alter) * share / A, 'random')
        within(counts['original'], n_sel, p_orig, 'original')
    return counts


def _valid_tokens(n_rows, length, alphabet, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(4, 24, (n_rows, length), generator=g)
    t[:, 0] = alphabet.cls_idx
    lens = torch.randint(length // 2, length, (n_rows,), generator=g)
    for i, n in enumerate(lens.tolist()):
        t[i, n] = alphabet.eos_idx
        t[i, n + 1:] = alphabet.padding_idx
    return t


@pytest.mark.parametrize('alphabet_name', ('Alphabet', 'Alphabet3'))
def test_mask_tokens_properties_on_200000_tokens(alphabet_name):
    from esme import alphabet as A
    alphabet = getattr(A, alphabet_name)
    tokens = _valid_tokens(700, 400, alphabet, seed=5)
    special = (tokens == alphabet.cls_idx) | (tokens == alphabet.eos_idx) | (tokens == alphabet.padding_idx)
    assert int((~special).sum()) >= 200_000
    keep = tokens.clone()
    torch.manual_seed(1234)
    masked, mask = A.mask_tokens(tokens, 0.15, 0.1, alphabet=alphabet)
    assert torch.equal(tokens, keep), 'the input was modified'
    c = check_mask_properties(tokens, masked, mask, 0.15, 0.1, alphabet)
    print(f'{alphabet_name} 2-D: {c}')
    packed = tokens[~(tokens == alphabet.padding_idx)]
    masked, mask = A.mask_tokens(packed, 0.3, 0.2, alphabet=alphabet)          # 1-D packed, other rates
    print(f'{alphabet_name} 1-D: {check_mask_properties(packed, masked, mask, 0.3, 0.2, alphabet)}')
    # freq = 0: exactly one selection per row, on an eligible position; a packed batch is one row
    masked, mask = A.mask_tokens(tokens, 0.0, 0.1, alphabet=alphabet)
    check_mask_properties(tokens, masked, mask, None, None, alphabet)
    assert bool((mask.sum(dim=1) == 1).all())
    masked, mask = A.mask_tokens(packed, 0.0, 0.1, alphabet=alphabet)
    assert int(mask.sum()) == 1
    # nothing eligible: nothing selected; an empty tensor; a 3-D one
    only = torch.tensor([[alphabet.cls_idx, alphabet.eos_idx, alphabet.padding_idx]])
    masked, mask = A.mask_tokens(only, 0.5, 0.1, alphabet=alphabet)
    assert not bool(mask.any()) and torch.equal(masked, only)
    masked, mask = A.mask_tokens(torch.zeros(0, dtype=torch.int64), alphabet=alphabet)
    assert masked.numel() == 0 and mask.dtype == torch.bool
    with pytest.raises(ValueError):
        A.mask_tokens(torch.zeros(1, 2, 3, dtype=torch.int64))
    # alter = 0: every selection is <mask>; alter = 1: every selection is the original again
    masked, mask = A.mask_tokens(tokens, 0.15, 0.0, alphabet=alphabet)
    assert bool((masked[mask] == alphabet.mask_idx).all())
    masked, mask = A.mask_tokens(tokens, 0.15, 1.0, alphabet=alphabet)
    assert torch.equal(masked, tokens) and bool(mask.any())


def test_the_property_checker_holds_on_the_reference_output():
    """g16_mask_tokens.npz: what the reference's mask_tokens returned for three seeds (tests/golden/make_golden_mask_tokens.py).  The
    checker above passes on it, and it is not vacuous: it rejects the same data with a defect."""
    from esme.alphabet import Alphabet3
    path = os.path.join(ROOT, 'tests', 'golden', 'g16_mask_tokens.npz')
    assert os.path.getsize(path) < 1 << 20
    total = dict(valid=0, selected=0, mask=0, random=0, original=0)
    with np.load(path, allow_pickle=False) as z:
        assert all(z[k].dtype.kind in 'fiub' for k in z.files)
        freq, alter = float(z['freq']), float(z['alter'])
        sets = [tuple(torch.from_numpy(z[f's{s}_{k}']) for k in ('tokens', 'masked', 'mask')) for s in (0, 1, 2)]
    assert {t.ndim for t, _, _ in sets} == {1, 2}
    for tokens, masked, mask in sets:
        c = check_mask_properties(tokens.long(), masked.long(), mask, freq, alter, Alphabet3)
        total = {k: total[k] + c[k] for k in total}
    print(f'reference output, three seeds: {total}')
    assert total['selected'] > 9000
    tokens, masked, mask = (t.clone() for t in sets[0])
    with pytest.raises(AssertionError, match='special'):
        bad = mask.clone()
        bad[:, 0] = True
        check_mask_properties(tokens.long(), masked.long(), bad, freq, alter, Alphabet3)
    with pytest.raises(AssertionError, match='<mask>'):
        all_mask = torch.where(mask, torch.tensor(Alphabet3.mask_idx, dtype=masked.dtype), masked)
        check_mask_properties(tokens.long(), all_mask.long(), mask, freq, alter, Alphabet3)
    with pytest.raises(AssertionError, match='selected'):
        check_mask_properties(tokens.long(), masked.long(), mask, 0.25, alter, Alphabet3)


# ------------------------------------------------------------------ the datasets

def test_masked_dataset_items():
    from esme.alphabet import Alphabet3
    from esme.data import FastaDataset, FastaTokenDataset, MaskedFastaDataset, MaskedFastaTokenDataset
    torch.manual_seed(7)
    ds = MaskedFastaDataset(FASTA, mask_freq=0.2, alter_freq=0.05)
    plain = FastaDataset(FASTA)
    assert isinstance(ds, FastaDataset) and len(ds) == len(plain) > 1 and (ds.mask_freq, ds.alter_freq) == (0.2, 0.05)
    for i in range(len(ds)):
        tokens, masked, mask = ds[i]
        assert torch.equal(tokens, plain[i]) and tokens.ndim == 2 and tokens.shape[0] == 1 and tokens.dtype == masked.dtype == torch.int64
        assert int(mask.sum()) > 0
        check_mask_properties(tokens, masked, mask, None, None, Alphabet3)
    batch = next(iter(ds.to_dataloader(batch_size=len(ds))))
    tokens, masked, mask = batch
    assert tokens.shape == masked.shape == mask.shape and tokens.shape[0] == len(ds) and mask.dtype == torch.bool
    assert torch.equal(tokens, plain.collate_fn([plain[i] for i in range(len(plain))]))
    check_mask_properties(tokens, masked, mask, None, None, Alphabet3)
    kw = dict(token_per_batch=1000, shuffle=True, random_state=3)
    td, tp = MaskedFastaTokenDataset(FASTA, **kw), FastaTokenDataset(FASTA, **kw)
    assert isinstance(td, FastaTokenDataset) and len(td) == len(tp) > 1 and (td.mask_freq, td.alter_freq) == (0.15, 0.1)
    for i, item in enumerate(td.to_dataloader()):
        tokens, (cu_lens, max_len), masked, mask = item
        assert torch.equal(tokens, tp[i][0]) and torch.equal(cu_lens, tp[i][1][0]) and int(max_len) == tp[i][1][1]
        assert tokens.ndim == 1 and masked.shape == mask.shape == tokens.shape and masked.dtype == torch.int64 and mask.dtype == torch.bool
        assert cu_lens.dtype == torch.int32 and int(cu_lens[-1]) == tokens.numel() and int(mask.sum()) > 0
        check_mask_properties(tokens, masked, mask, None, None, Alphabet3)
    td2 = MaskedFastaTokenDataset(FASTA, None, 1000, None, None, 0.5, 0.0, False, False, None, Alphabet3)      # the reference's positional order
    assert (td2.mask_freq, td2.alter_freq, td2.token_per_batch) == (0.5, 0.0, 1000)
    ds2 = MaskedFastaDataset(FASTA, None, None, None, 0.5, 0.0, Alphabet3)
    assert (ds2.mask_freq, ds2.alter_freq) == (0.5, 0.0)


# ------------------------------------------------------------------ the fixture of tests/test_mlm_train_gpu.py

def test_embed_grad_fixture_is_consistent():
    from golden_util import GOLDEN, load_golden
    from esme import synthetic as syn
    path = os.path.join(GOLDEN, 'g17_embed_grad.npz')
    assert os.path.getsize(path) < 1 << 20
    with np.load(path, allow_pickle=False) as z:
        assert all(z[k].dtype.kind in 'fiub' for k in z.files)
    g, g13, g15 = load_golden('g17_embed_grad.npz'), load_golden('g13_lora.npz'), load_golden('g15_full_grad.npz')
    for kind in ('esm2', 'esmc'):
        L, E, seed = (int(g13[f'{kind}_{k}']) for k in ('L', 'E', 'seed'))
        table = syn.synthetic_state_dict(kind, L, E, seed)['embed_tokens.weight']
        truth = g[f'{kind}_oracle/embed_tokens.weight']
        assert truth.shape == table.shape and truth.dtype == torch.float64
        assert abs(g[f'{kind}_oracle/loss'] - g15[f'{kind}_oracle/loss']) < 1e-12          # the same step as the full-gradient fixture
        assert 1e-3 < g[f'{kind}_bf16_error/embed_tokens.weight'] < 5e-2
        rows = g[f'{kind}_rows']
        assert torch.equal(rows.long(), torch.bincount(g15[f'{kind}_tokens_in'], minlength=table.shape[0]))
        zero = truth.abs().amax(dim=1) == 0
        assert bool(zero[rows == 0].all()) and bool((~zero)[(rows > 0) & (torch.arange(rows.numel()) != 32)].all())
        assert int(rows[32]) > 0 and bool(zero[32]) == (kind == 'esm2')                    # ESM-2 zeroes <mask> rows, ESM-C trains them
    src = open(os.path.join(GOLDEN, 'make_golden_embed_grad.py')).read()
    assert 'import_reference' not in src and 'make_golden as' not in src                  # the oracle only


# ------------------------------------------------------------------ the opt-in on a CPU model

@pytest.mark.parametrize('kind', ('esm2', 'esmc'))
def test_mark_trainable_embedding_flag(tmp_path, kind):
    from esme import ESM, synthetic as syn
    path = syn.write_checkpoint(str(tmp_path / f'{kind}.safetensors'), f'{kind}_t', 2, 64, 2, seed=5)
    model = ESM.from_pretrained(path, device='cpu')
    keys = list(model.state_dict())
    w = model.embed_tokens.weight
    flags = lambda: {n for n, p in model.named_parameters() if p.requires_grad}
    assert not w.requires_grad
    base = flags() if model.mark_trainable() is model else None
    assert 'embed_tokens.weight' not in base
    assert model.mark_trainable(embedding=True) is model and flags() == base | {'embed_tokens.weight'}
    assert flags() == base | {'embed_tokens.weight'} and model.__dict__['_train_embedding'] is True
    assert model.mark_trainable(False, False, embedding=True) is model and flags() == {'embed_tokens.weight'}
    model.mark_trainable()                                                    # the default withdraws the opt-in and the flag it set
    assert flags() == base and '_train_embedding' not in model.__dict__
    w.requires_grad_(True)                                                    # a flag set by hand: not touched, and still refused
    model.mark_trainable()
    assert w.requires_grad and '_train_embedding' not in model.__dict__
    with pytest.raises(NotImplementedError, match='mark_trainable'):
        model.forward_trainable(torch.zeros(4, dtype=torch.long), (torch.tensor([0, 4], dtype=torch.int32), 4))
    model.mark_trainable(embedding=True).mark_trainable(embedding=False)
    assert not w.requires_grad
    assert list(model.state_dict()) == keys
    model.mark_trainable(embedding=True).set_precision('exact')
    with pytest.raises(NotImplementedError, match="precision"):
        model.forward_trainable(torch.zeros(4, dtype=torch.long), (torch.tensor([0, 4], dtype=torch.int32), 4))


def test_standing_refusals_with_the_opt_in():
    """What forward_trainable refused before the opt-in existed, it refuses with it, by name; the checks need no device."""
    from esme import ESM1b, ESM2
    tok, pad = torch.full((4,), 5, dtype=torch.long), (torch.tensor([0, 4], dtype=torch.int32), 4)
    make = lambda cls=ESM2, **kw: cls(**{'num_layers': 1, 'embed_dim': 128, 'attention_heads': 4, **kw}).mark_trainable(embedding=True)
    for m, pat in ((make(embed_dim=480, attention_heads=20), 'padded layout'), (make(ESM1b, attention_heads=2), 'learned-position')):
        with pytest.raises(NotImplementedError, match=pat):
            m.forward_trainable(tok, pad)
    m = make()
    for precision in ('high', 'half', 'exact'):
        m.precision = precision
        with pytest.raises(NotImplementedError, match=f"precision '{precision}'"):
            m.forward_trainable(tok, pad)
    m.precision = 'fast'
    m.mark_trainable(False, False, embedding=True)
    m.quantization = '8bit'
    m._qlora = True                                                        # even where adapters may train over a quantised base
    with pytest.raises(NotImplementedError, match='embedding=True.*quantised'):
        m.forward_trainable(tok, pad)
    with pytest.raises(NotImplementedError, match='quantised'):
        m.mark_trainable(embedding=True)
    m.quantization, m._qlora = None, False
    with pytest.raises(RuntimeError, match='no CPU fallback'):               # every check passed: the first kernel call says where it must run
        m.forward_trainable(tok, pad)
    with pytest.raises(TypeError):
        m.mark_trainable(embeddings=True)
