"""What tests/test_extreme_shapes_train_gpu.py relies on, shown without a device.

The comparators reject what they are for: with the modules' no-defect emulations as a stand-in "kernel output" on a reduced batch
(the launch limit scaled down to a parameter, the checks' logic the same), the checks of section A fail for an output whose
sequences from `grid_z` on were left at their prefill and for one that computed them from sequence b - grid_z, and the checks of
section B fail for an output whose rows at an element offset >= 2^31 were read 2^31 elements too early; all pass for the unmodified
stand-in.  And the bounds admit a correct kernel at the new shapes: the emulations lie inside the modules' bounds on the lengths
(2100, 65, 1) at H = 1, d in {32, 64}, and on the picks of the 70 002-sequence batch.
"""
import numpy as np
import pytest
import torch

import attn_bwd_bounds as AB
import attn_map_bounds as MB
import contact_bounds as CB
import contact_feature_bounds as FB
import extreme_shapes as XS

NAN = float('nan')
GRID_Z, SPLIT = 20, 12             # the reduced batch: 30 sequences, launches of at most 20, sub-batches [0, 12) and [12, 30)
WIDE = (2100, 65, 1)
WIDE_LD = 1 << 20


def _small_lengths():
    rng = np.random.Generator(np.random.PCG64(2))
    return [70] + rng.integers(1, 9, size=28).tolist() + [70]


def test_inputs():
    lengths = XS.many_lengths()
    assert len(lengths) == 70002 and lengths[0] == lengths[-1] == 300 and set(lengths[1:-1]) == set(range(1, 9))
    rows = XS.row_lengths()
    assert len(rows) == 70002 and set(rows) == set(range(13))
    p = XS.picks(70002)
    assert p == sorted(set(p)) and {0, 1, 70001} | set(range(65533, 65541)) <= set(p) and len(p) >= 45
    assert XS.picks(30, grid_z=GRID_Z, extra=5)[-1] == 29
    c = XS.crossing(WIDE, WIDE_LD)
    assert c == dict(first_row=2048, sequences=[1, 2], inside=[(0, 2048)])
    assert XS.crossing([66000, 2700, 300, 1], 32768)['sequences'] == [1, 2, 3]
    with pytest.raises(AssertionError):
        XS.crossing(WIDE, 1 << 19)                                  # nothing past 2^31
    with pytest.raises(AssertionError):
        XS.crossing((4100, 5), WIDE_LD)                             # a sequence past 2^32
    x = torch.arange(12.0).view(6, 2)
    got, cu = XS.sub_batch(x, XS.cu_of([1, 2, 0, 3]), [3, 1])
    assert torch.equal(got, x[[3, 4, 5, 1, 2]]) and cu.tolist() == [0, 3, 5] and cu.dtype == torch.int32


def test_comparators():
    a = torch.tensor([[1.0, NAN], [0.0, 2.0]])
    XS.assert_rows_equal(a, a.clone(), 'same')
    with pytest.raises(AssertionError, match='1 of 2 rows differ, the first at 1'):
        XS.assert_rows_equal(a, torch.tensor([[1.0, NAN], [-0.0, 2.0]]), '-0')
    with pytest.raises(AssertionError):
        XS.assert_rows_equal(a, a.double(), 'dtype')
    ref, bound = torch.tensor([1.0, 2.0, 0.0]).double(), torch.tensor([0.1, 0.1, 0.0]).double()
    assert XS.assert_inside(torch.tensor([1.05, 2.0, 0.0]), ref, bound, 'inside') == pytest.approx(0.5, rel=1e-3)
    for bad in ([1.2, 2.0, 0.0], [1.0, 2.0, 1e-30], [1.0, NAN, 0.0], [1.0, float('inf'), 0.0]):
        with pytest.raises(AssertionError):
            XS.assert_inside(torch.tensor(bad), ref, bound, 'outside')
    buf = torch.full((10, 16), 0x5A5A, dtype=torch.int16).view(torch.bfloat16)
    buf[2:7, 4:8] = 1.0
    XS.assert_untouched(buf, 0x5A5A, (2, 7), [(4, 8)], 'clean', chunk=4)
    for r, c in ((1, 5), (7, 5), (3, 3), (3, 8), (9, 15)):
        dirty = buf.clone()
        dirty[r, c] = 1.0
        with pytest.raises(AssertionError):
            XS.assert_untouched(dirty, 0x5A5A, (2, 7), [(4, 8)], 'dirty', chunk=4)


# ------------------------------------------------------------------ section A's checks on a reduced batch

def _section_a(full, starts, run_part, run_alone, reference, which, B, what):
    """The three conditions of section A, as the GPU file applies them"""
    XS.assert_split_identity(full, starts, run_part, B, what, split=SPLIT)
    alone = run_alone()
    XS.assert_picks_identity(full, starts, alone, which, what)
    ref, bound = reference()
    XS.assert_inside(alone, ref, bound, what)


def _wrong_outputs(full, starts, B):
    """(a) sequences from GRID_Z on left at the prefill; (b) those sequences computed from sequence b - GRID_Z (its elements, repeated
    or cut to the size sequence b owns)."""
    a, b = full.clone(), full.clone()
    for s in range(GRID_Z, B):
        lo, hi = starts[s], starts[s + 1]
        a[lo:hi] = NAN
        src = full[starts[s - GRID_Z]:starts[s - GRID_Z + 1]]
        if hi > lo:
            b[lo:hi] = 0.0 if not src.shape[0] else src.repeat(-(-(hi - lo) // src.shape[0]), *([1] * (src.dim() - 1)))[:hi - lo]
    assert not XS._bits(b).equal(XS._bits(full))
    return {'prefill': a, 'b - grid_z': b}


def test_section_a_checks_reject_an_ignored_b0_rows():
    """attn_varlen_bwd's emulation as the stand-in: an output in rows"""
    H, d = 2, 32
    lengths = _small_lengths()
    B = len(lengths)
    c = AB.make_operands(lengths, H, d, seed=5)
    o = AB.forward_bf16(c['q'], c['k'], c['v'], c['cu'], H, d, c['scale'])
    ops = tuple(t.contiguous() for t in (c['q'], c['k'], c['v'], o, c['do']))
    cu = c['cu']
    which = XS.picks(B, grid_z=GRID_Z, extra=5)
    emu = lambda x, cu_: torch.cat(AB.emulate_bwd(*x, cu_, H, d, c['scale']), 1)
    full = emu(ops, cu)
    starts = cu.tolist()
    part = lambda a, b: emu(tuple(t[starts[a]:starts[b]] for t in ops), (cu[a:b + 1] - cu[a]).to(torch.int32))
    sub, cs = XS.sub_batch(ops, cu, which)

    def reference():
        ref = AB.reference_bwd(sub[0], sub[1], sub[2], sub[4], cs, H, d, c['scale'])[:3]
        return torch.cat(ref, 1), torch.cat(AB.bwd_bound(*sub, cs, H, d, c['scale']), 1)
    check = lambda out: _section_a(out, starts, part, lambda: emu(sub, cs), reference, which, B, 'attn_varlen_bwd stand-in')
    check(full)
    for name, wrong in _wrong_outputs(full, starts, B).items():
        with pytest.raises(AssertionError):
            check(wrong)
        # the picks alone do not see the full run: only the identities can tell, and each does
        with pytest.raises(AssertionError):
            XS.assert_split_identity(wrong, starts, part, B, name, split=SPLIT)
        with pytest.raises(AssertionError):
            XS.assert_picks_identity(wrong, starts, emu(sub, cs), which, name)


def test_section_a_checks_reject_an_ignored_b0_maps():
    """contact_layer's emulation as the stand-in: a packed output of maps, where sequences of 1 and 2 rows own nothing"""
    H, d = 2, 16
    lengths = _small_lengths()
    B = len(lengths)
    layers, cu, scale = CB.make_operands(lengths, H, d, seed=6)
    w = torch.tensor([[0.7, -1.1], [-0.4, 0.9]])
    which = XS.picks(B, grid_z=GRID_Z, extra=5)
    emu = lambda lay, cu_: torch.cat([m.reshape(-1) for m in CB.emulate_contacts(lay, cu_, H, d, scale, w, -0.75)])
    full = emu(layers, cu)
    cul = cu.tolist()
    starts = np.concatenate(([0], np.cumsum([max(n - 2, 0) ** 2 for n in lengths]))).tolist()
    part = lambda a, b: emu([(q[cul[a]:cul[b]], k[cul[a]:cul[b]], qp) for q, k, qp in layers], (cu[a:b + 1] - cu[a]).to(torch.int32))
    subs = [XS.sub_batch((q, k), cu, which) for q, k, _ in layers]
    cs = subs[0][1]
    sub_layers = [(qk[0], qk[1], False) for qk, _ in subs]

    def reference():
        flat = lambda maps: torch.cat([m.reshape(-1) for m in maps])
        return flat(CB.reference_contacts(sub_layers, cs, H, d, scale, w, -0.75)), flat(CB.contact_bound(sub_layers, cs, H, d, scale, w, -0.75))
    check = lambda out: _section_a(out, starts, part, lambda: emu(sub_layers, cs), reference, which, B, 'contact_layer stand-in')
    check(full)
    for name, wrong in _wrong_outputs(full, starts, B).items():
        with pytest.raises(AssertionError):
            check(wrong)


# ------------------------------------------------------------------ section B: the wide shape

_WIDE = {}


def _wide_bwd(d):
    if d not in _WIDE:
        c = AB.make_operands(WIDE, 1, d, seed=7 + d)
        o = AB.forward_bf16(c['q'], c['k'], c['v'], c['cu'], 1, d, c['scale'])
        ops = tuple(t.contiguous() for t in (c['q'], c['k'], c['v'], o, c['do']))
        ref = AB.reference_bwd(ops[0], ops[1], ops[2], ops[4], c['cu'], 1, d, c['scale'])[:3]
        bound = AB.bwd_bound(*ops, c['cu'], 1, d, c['scale'])
        _WIDE[d] = dict(ops=ops, cu=c['cu'], scale=c['scale'], ref=torch.cat(ref, 1), bound=torch.cat(bound, 1))
    return _WIDE[d]


@pytest.mark.parametrize('d', (32, 64))
def test_attn_bwd_bound_admits_the_emulation_on_the_wide_shape(d):
    c = _wide_bwd(d)
    got = torch.cat(AB.emulate_bwd(*c['ops'], c['cu'], 1, d, c['scale']), 1)
    XS.assert_inside(got, c['ref'], c['bound'], f'attn_varlen_bwd emulation, lengths {WIDE}, d{d}')


def test_section_b_checks_reject_a_truncated_offset():
    """(c): every packed row at an element offset >= 2^31 of the (2166, 2^20) buffer read 2^31 elements, i.e. 2048 rows, too early."""
    d = 32
    c = _wide_bwd(d)
    first = XS.crossing(WIDE, WIDE_LD)['first_row']
    emu = lambda ops: torch.cat(AB.emulate_bwd(*ops, c['cu'], 1, d, c['scale']), 1)
    plain = emu(c['ops'])
    XS.assert_rows_equal(emu(c['ops']), plain, 'unmodified')
    wrapped = tuple(torch.cat((t[:first], t[:t.shape[0] - first])) for t in c['ops'])
    wrong = emu(wrapped)
    with pytest.raises(AssertionError):
        XS.assert_rows_equal(wrong, plain, 'truncated offsets against contiguous operands')
    with pytest.raises(AssertionError):
        XS.assert_inside(wrong, c['ref'], c['bound'], 'truncated offsets against float64')
    # the sequences that start past 2^31, on their own rows: both checks still tell
    a = int(c['cu'][1])
    with pytest.raises(AssertionError):
        XS.assert_rows_equal(wrong[a:], plain[a:], 'sequences past 2^31')
    with pytest.raises(AssertionError):
        XS.assert_inside(wrong[a:], c['ref'][a:], c['bound'][a:], 'sequences past 2^31 against float64')


@pytest.mark.parametrize('d', (32, 64))
def test_observer_bounds_admit_the_emulations_on_the_wide_shape(d):
    layers, cu, scale = CB.make_operands(WIDE, 1, d, seed=8 + d)
    w = torch.tensor([[0.8], [-1.3]])
    flat = lambda maps: torch.cat([m.reshape(-1) for m in maps])
    XS.assert_inside(flat(CB.emulate_contacts(layers, cu, 1, d, scale, w, -0.75)), flat(CB.reference_contacts(layers, cu, 1, d, scale, w, -0.75)),
                     flat(CB.contact_bound(layers, cu, 1, d, scale, w, -0.75)), f'contact_layer emulation, lengths {WIDE}, d{d}')
    pairs = FB.make_pairs(WIDE, seed=d)
    XS.assert_inside(FB.emulate_features(layers, cu, 1, d, scale, pairs), FB.reference_features(layers, cu, 1, d, scale, pairs),
                     FB.feature_bound(layers, cu, 1, d, scale, pairs), f'contact_features emulation, lengths {WIDE}, d{d}')
    mlayers, mcu, mscale = MB.make_operands(WIDE, 1, d, seed=9 + d)
    XS.assert_inside(flat(MB.emulate_maps(mlayers, mcu, 1, d, mscale, [0])), flat(MB.reference_maps(mlayers, mcu, 1, d, mscale, [0])),
                     flat(MB.map_bound(mlayers, mcu, 1, d, mscale, [0])), f'attn_maps emulation, lengths {WIDE}, d{d}')


def test_bounds_admit_the_emulations_on_the_picks_of_the_large_batch():
    lengths = XS.many_lengths()
    sub = [lengths[i] for i in XS.picks(len(lengths))]
    assert sub[0] == sub[-1] == 300 and len(sub) >= 45
    H, d = 2, 32
    c = AB.make_operands(sub, H, d, seed=11)
    o = AB.forward_bf16(c['q'], c['k'], c['v'], c['cu'], H, d, c['scale'])
    got = AB.emulate_bwd(c['q'], c['k'], c['v'], o, c['do'], c['cu'], H, d, c['scale'])
    ref = AB.reference_bwd(c['q'], c['k'], c['v'], c['do'], c['cu'], H, d, c['scale'])[:3]
    XS.assert_inside(list(got), list(ref), list(AB.bwd_bound(c['q'], c['k'], c['v'], o, c['do'], c['cu'], H, d, c['scale'])), 'attn_varlen_bwd emulation, picks')
    layers, cu, scale = CB.make_operands(sub, H, d, seed=12)
    w = torch.tensor([[0.7, -1.1], [-0.4, 0.9]])
    XS.assert_inside(CB.emulate_contacts(layers, cu, H, d, scale, w, -0.75), CB.reference_contacts(layers, cu, H, d, scale, w, -0.75),
                     CB.contact_bound(layers, cu, H, d, scale, w, -0.75), 'contact_layer emulation, picks')
    pairs = FB.make_pairs(sub, seed=3)
    XS.assert_inside(FB.emulate_features(layers, cu, H, d, scale, pairs), FB.reference_features(layers, cu, H, d, scale, pairs),
                     FB.feature_bound(layers, cu, H, d, scale, pairs), 'contact_features emulation, picks')
    mlayers, mcu, mscale = MB.make_operands(sub, H, d, seed=13)
    for weights, bf16 in ((None, False), (torch.tensor([[0.75, -1.5]]), True)):
        XS.assert_inside(MB.emulate_maps(mlayers, mcu, H, d, mscale, [1, 0], weights, out_bf16=bf16), MB.reference_maps(mlayers, mcu, H, d, mscale, [1, 0], weights),
                         MB.map_bound(mlayers, mcu, H, d, mscale, [1, 0], weights, out_bf16=bf16), f'attn_maps emulation, picks, weighted {weights is not None}')
