"""The backward and observer kernels past the limits tests/test_extreme_shapes_gpu.py holds the inference path to: more than 65 535
sequences in one batch (the kernels that take the sequence from grid z launch in chunks and index with b0 + blockIdx.z; a second
launch runs on such a batch only) and row offsets past 2^31 elements, between sequences (64-bit products) and inside one sequence
(unsigned 32-bit products, valid to 2^32).

 A. B = 70 002 on contiguous operands: attn_varlen_bwd, contact_layer, contact_features, attn_maps -- every sequence bit-equal to the
    same sequence inside one of two sub-batches that are one launch each, the picks (tests/extreme_shapes.picks) bit-equal to the
    picks alone and inside the module's float64 bound; attn_pool_bwd and segment_mean_bwd on 70 002 sequences of 0 to 12 rows.
 B. One (2166, 2^20) bfloat16 buffer, lengths (2100, 65, 1), every operand a column block of it: rows 2048 .. 2099 of the first
    sequence lie 2^31 .. 2^32 elements from its first row, the other two sequences start past element 2^31.  Inside the bound, and
    bit-equal to the same operands in contiguous tensors.
 C. The row kernels (embed_bwd, segment_mean_bwd, attn_pool_bwd, dequantize_*_t) on column blocks of a buffer whose rows pass 2^31.
 D. Whole models over 70 000 peptides: predict_contacts, contact_features, attention_maps, and forward_trainable + backward against
    the oracle's float64 step on the picks.

References and bounds are the modules' own (attn_bwd_bounds, contact_bounds, contact_feature_bounds, attn_map_bounds,
attn_pool_bwd_bounds, embed_bwd_bounds, segment_mean_bwd_bounds), unchanged, at ratio <= 1.0; tests/test_extreme_shapes_train_cpu.py
shows that they admit a correct kernel at these shapes and that the checks used here reject an ignored b0 and a truncated offset.
Every output holds NaN (or the module's PREFILL) before the call.  profiles/extreme_shapes_train.txt keeps one run's printed ratios.

Left out: the fused AdamW on one tensor of more than 2^31 elements (parameter, gradient, master and two moments: ~36 GB; the header
caps a chunk at 2^31 and the chunk arithmetic is plain int64_t), and segment_mean_bwd's float32 instance past 2^31 (the same
(70 000, 32 768) buffer in float32 is twice the 4.6 GB a test here may hold).
"""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import attn_bwd_bounds as AB
import attn_map_bounds as MB
import attn_pool_bwd_bounds as PB
import contact_bounds as CB
import contact_feature_bounds as FB
import embed_bwd_bounds as EB
import extreme_shapes as XS
import segment_mean_bwd_bounds as SB

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF, F32 = torch.bfloat16, torch.float32
NAN = float('nan')
BIAS = -0.75
CANARY = 0x5A5A
WIDE = (2100, 65, 1)               # section B: one sequence past 2^31 elements inside itself, two that start past 2^31
WIDE_LD = 1 << 20


@pytest.fixture(autouse=True)
def _threads_and_memory():
    torch.set_num_threads(16)
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _randn(shape, seed, dtype=BF, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV) * scale).to(dtype)


def _starts(sizes):
    """(B + 1) python ints: where each sequence's elements begin in a packed output"""
    return np.concatenate(([0], np.cumsum(np.asarray(sizes, dtype=np.int64)))).tolist()


def _blocks(flat, starts, shapes):
    return [flat[a:a + math.prod(s)].view(s) for a, s in zip(starts, shapes)]


def test_the_batch_is_the_inference_suites():
    from test_extreme_shapes_gpu import GRID_Z, many_lengths
    assert XS.many_lengths() == many_lengths() and XS.GRID_Z == GRID_Z
    lengths = XS.many_lengths()
    assert len(lengths) == 70002 > XS.GRID_Z and max(XS.SPLIT, len(lengths) - XS.SPLIT) < XS.GRID_Z        # each sub-batch is one launch
    p = XS.picks(len(lengths))
    assert {0, 1, len(lengths) - 1} | set(range(65533, 65541)) <= set(p) and len(p) >= 40
    rows = XS.row_lengths()
    assert len(rows) == 70002 and min(rows) == 0 and max(rows) == 12 and 0 in rows[XS.GRID_Z:]


# ====================================================================== A. more than 65 535 sequences

def _many():
    lengths = XS.many_lengths()
    return lengths, XS.cu_of(lengths), XS.picks(len(lengths))


def _sub(cu, a, b):
    """cu_lens (device) of the sequences a .. b - 1 and their row range"""
    lo, hi = int(cu[a]), int(cu[b])
    return (cu[a:b + 1] - lo).to(torch.int32).to(DEV), lo, hi


# ---------------------------------------------------------------------- A1

def _attn_bwd(q, k, v, o, do, cu, max_len, H, scale):
    """(T, 3 E): dq | dk | dv of one call into NaN-filled contiguous tensors"""
    from esme import _hip_attn_bwd as HB
    outs = tuple(torch.full_like(q, NAN) for _ in range(3))
    HB.attn_varlen_bwd(q, k, v, o, do, cu, max_len, H, scale, *outs)
    return torch.cat(outs, 1)


@pytest.mark.parametrize('d', (32, 64))
def test_attn_varlen_bwd_more_than_65535_sequences(d):
    from esme import _hip
    H = 2
    E, scale = H * d, d ** -0.5
    lengths, cu, which = _many()
    B, T = len(lengths), sum(lengths)
    q, k, v = (_randn((T, E), 100 + d + i, scale=math.sqrt(1.5)) for i in range(3))
    do = _randn((T, E), 200 + d)
    cud = cu.to(DEV)
    o = _hip.attn_varlen(q, k, v, cud, max(lengths), H, softmax_scale=scale)
    full = _attn_bwd(q, k, v, o, do, cud, max(lengths), H, scale)
    assert not bool(torch.isnan(full).any()), 'rows of a sequence were left unwritten'
    what = f'attn_varlen_bwd d{d} B={B}'

    def part(a, b):
        c, lo, hi = _sub(cu, a, b)
        return _attn_bwd(q[lo:hi], k[lo:hi], v[lo:hi], o[lo:hi], do[lo:hi], c, max(lengths[a:b]), H, scale)
    XS.assert_split_identity(full, cu.tolist(), part, B, what)
    (qs, ks, vs, os_, dos), cs = XS.sub_batch((q, k, v, o, do), cu, which)
    ml = max(lengths[i] for i in which)
    alone = _attn_bwd(qs, ks, vs, os_, dos, cs.to(DEV), ml, H, scale)
    XS.assert_picks_identity(full, cu.tolist(), alone, which, what)
    cpu = [t.cpu() for t in (qs, ks, vs, os_, dos)]
    ref = AB.reference_bwd(cpu[0], cpu[1], cpu[2], cpu[4], cs, H, d, scale)[:3]
    bound = AB.bwd_bound(cpu[0], cpu[1], cpu[2], cpu[3], cpu[4], cs, H, d, scale)
    for i, name in enumerate(('dq', 'dk', 'dv')):
        XS.assert_inside(alone[:, i * E:(i + 1) * E].cpu(), ref[i], bound[i], f'{what} {name}, {len(which)} picks')


# ---------------------------------------------------------------------- A2

def _contact_weights(L, H, seed=5):
    w = torch.randn(L, H, generator=torch.Generator().manual_seed(seed))
    assert bool((w > 0).any()) and bool((w < 0).any())
    return w.to(DEV)


def _contacts(layers, cu, max_len, H, d, scale, w, f=1, e=1):
    """The packed fp32 map of one contact_layer call per layer (`init`, then accumulate) on a NaN-filled map with one sentinel element
    behind it and a 0xFF-filled workspace; the sequences' ranges tile the map, so the sentinel is all that lies outside them."""
    from esme import _hip, _hip_contacts as HC
    n, off, total = HC.map_offsets(cu, f, e)
    buf = torch.full((total + 1,), NAN, dtype=F32, device=DEV)
    buf[total] = -7.0
    out = buf[:total]
    ws = torch.full((max(HC.workspace_bytes(cu.numel() - 1, int(cu[-1]), H), 16),), 0xFF, dtype=torch.uint8, device=DEV)
    with _hip.stream_scope(DEV):
        for l, (q, k, qp) in enumerate(layers):
            HC.contact_layer(q, k, cu, max_len, H, d, scale, w[l].contiguous(), BIAS, l == 0, out, off, ws, q_prescaled=qp, trim_front=f, trim_back=e)
    torch.cuda.synchronize()
    assert float(buf[total]) == -7.0, 'the element behind the last map was written'
    assert not bool(torch.isnan(out).any()), 'an owned map element was left unwritten'
    return out


@pytest.mark.parametrize('d', (16, 64))
def test_contact_layer_more_than_65535_sequences(d):
    H, L = 2, 2
    E, scale = H * d, d ** -0.5
    lengths, cu, which = _many()
    B, T = len(lengths), sum(lengths)
    layers = [(_randn((T, E), 300 + d + 2 * l, scale=math.sqrt(1.5)), _randn((T, E), 301 + d + 2 * l, scale=math.sqrt(1.5)), False) for l in range(L)]
    w = _contact_weights(L, H)
    n = [max(s - 2, 0) for s in lengths]                   # sequences of 1 and 2 rows are trimmed to nothing and own no element
    assert n.count(0) > 10000
    starts = _starts([m * m for m in n])
    full = _contacts(layers, cu.to(DEV), max(lengths), H, d, scale, w)
    assert full.numel() == starts[-1]
    what = f'contact_layer d{d} B={B}'

    def part(a, b):
        c, lo, hi = _sub(cu, a, b)
        return _contacts([(q[lo:hi], k[lo:hi], qp) for q, k, qp in layers], c, max(lengths[a:b]), H, d, scale, w)
    XS.assert_split_identity(full, starts, part, B, what)
    sub = [XS.sub_batch((q, k), cu, which) for q, k, _ in layers]
    cs = sub[0][1]
    sub_layers = [(qk[0], qk[1], False) for qk, _ in sub]
    alone = _contacts(sub_layers, cs.to(DEV), max(lengths[i] for i in which), H, d, scale, w)
    XS.assert_picks_identity(full, starts, alone, which, what)
    cpu_layers = [(q.cpu(), k.cpu(), qp) for q, k, qp in sub_layers]
    ref = CB.reference_contacts(cpu_layers, cs, H, d, scale, w.cpu(), BIAS)
    bound = CB.contact_bound(cpu_layers, cs, H, d, scale, w.cpu(), BIAS)
    got = _blocks(alone.cpu(), _starts([r.numel() for r in ref]), [tuple(r.shape) for r in ref])
    XS.assert_inside(got, ref, bound, f'{what}, {len(which)} picks')


# ---------------------------------------------------------------------- A3

SENTINEL = -12345.0


def _features(layers, cu, max_len, H, d, scale, pairs, f=1, e=1):
    from esme import _hip, _hip_contact_features as HF
    feat = torch.full((pairs.shape[0], len(layers) * H), SENTINEL, dtype=F32, device=DEV)
    ws = torch.full((max(HF.workspace_bytes(cu.numel() - 1, int(cu[-1]), H), 16),), 0xFF, dtype=torch.uint8, device=DEV)
    with _hip.stream_scope(DEV):
        for l, (q, k, qp) in enumerate(layers):
            HF.contact_features(q, k, cu, max_len, H, d, scale, pairs, feat, l * H, ws, q_prescaled=qp, trim_front=f, trim_back=e)
    torch.cuda.synchronize()
    return feat


def test_contact_features_more_than_65535_sequences():
    H, d, L = 3, 32, 2
    E, scale = H * d, d ** -0.5
    lengths, cu, which = _many()
    B, T = len(lengths), sum(lengths)
    layers = [(_randn((T, E), 400 + 2 * l, scale=math.sqrt(1.5)), _randn((T, E), 401 + 2 * l, scale=math.sqrt(1.5)), False) for l in range(L)]
    n = [max(s - 2, 0) for s in lengths]
    # the picks' pairs (contact_feature_bounds.make_pairs, renumbered to the whole batch), then pair (0, 0) of EVERY sequence that keeps a
    # row, so that no sequence is left out of the identity, then three rows out of range
    own = FB.make_pairs([lengths[i] for i in which], seed=3)
    renumbered = own.clone()
    renumbered[:, 0] = torch.tensor(which, dtype=torch.int32)[own[:, 0].long()]
    assert int(renumbered[:, 0].max()) >= XS.GRID_Z
    every = torch.tensor([[s, 0, 0] for s in range(B) if n[s] > 0], dtype=torch.int32)
    far = next(i for i in which if i >= XS.GRID_Z and n[i] > 0)
    bad = torch.tensor([[B, 0, 0], [far, n[far], 0], [B - 1, 0, n[B - 1]]], dtype=torch.int32)
    pairs = torch.cat((renumbered, every, bad)).contiguous()
    P0, P1 = own.shape[0], own.shape[0] + every.shape[0]
    full = _features(layers, cu.to(DEV), max(lengths), H, d, scale, pairs.to(DEV))
    assert bool(torch.isnan(full[P1:]).all()), 'an out-of-range pair did not give a NaN row'
    assert bool(torch.isfinite(full[:P1]).all())
    what = f'contact_features d{d} B={B}'
    for a, b in XS.halves(B):
        c, lo, hi = _sub(cu, a, b)
        sel = ((pairs[:P1, 0] >= a) & (pairs[:P1, 0] < b)).nonzero().reshape(-1)
        sub_pairs = pairs[sel].clone()
        sub_pairs[:, 0] -= a
        got = _features([(q[lo:hi], k[lo:hi], qp) for q, k, qp in layers], c, max(lengths[a:b]), H, d, scale, sub_pairs.contiguous().to(DEV))
        XS.assert_rows_equal(full[sel.to(DEV)], got, f'{what}: the pairs of sequences [{a}, {b}) in the whole batch against the sub-batch')
    sub = [XS.sub_batch((q, k), cu, which) for q, k, _ in layers]
    cs = sub[0][1]
    sub_layers = [(qk[0], qk[1], False) for qk, _ in sub]
    alone = _features(sub_layers, cs.to(DEV), max(lengths[i] for i in which), H, d, scale, own.to(DEV))
    XS.assert_rows_equal(full[:P0], alone, f'{what}: the picks packed in the whole batch against the picks alone')
    cpu_layers = [(q.cpu(), k.cpu(), qp) for q, k, qp in sub_layers]
    ref = FB.reference_features(cpu_layers, cs, H, d, scale, own)
    bound = FB.feature_bound(cpu_layers, cs, H, d, scale, own)
    XS.assert_inside(alone.cpu(), ref, bound, f'{what}, {P0} pairs of {len(which)} picks')


# ---------------------------------------------------------------------- A4

def _maps(layer, cu, max_len, H, d, scale, heads, weights=None, dtype=F32):
    """The packed map of one attn_maps call on a NaN-filled buffer and a 0xFF-filled workspace"""
    from esme import _hip, _hip_attn_maps as HM
    q, k, qp = layer
    n_out = 1 if weights is not None else len(heads)
    S, off, total = HM.map_offsets(cu, n_out)
    out = torch.full((max(total, 1),), NAN, dtype=dtype, device=DEV)
    ws = torch.full((max(HM.workspace_bytes(cu.numel() - 1, int(cu[-1]), len(heads)), 16),), 0xFF, dtype=torch.uint8, device=DEV)
    hl = torch.tensor(heads, dtype=torch.int32, device=DEV)
    w = None if weights is None else weights.to(device=DEV, dtype=F32).contiguous()
    with _hip.stream_scope(DEV):
        HM.attn_maps(q, k, cu, max_len, H, d, scale, hl, out, off, 0, ws, head_weights=w, q_prescaled=qp)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out[:total].float()).any()), 'an owned map element was left unwritten'
    return out[:total]


@pytest.mark.parametrize('mode', ('heads-fp32', 'weighted-bf16'))
@pytest.mark.parametrize('d', (32, 128))
def test_attn_maps_more_than_65535_sequences(d, mode):
    H, heads = 2, [1, 0]
    E, scale = H * d, d ** -0.5
    weights = torch.tensor([0.75, -1.5]) if mode == 'weighted-bf16' else None
    dtype = BF if mode == 'weighted-bf16' else F32
    n_out = 1 if weights is not None else len(heads)
    lengths, cu, which = _many()
    B, T = len(lengths), sum(lengths)
    layer = (_randn((T, E), 500 + d, scale=math.sqrt(3.0)), _randn((T, E), 501 + d, scale=math.sqrt(3.0)), False)
    starts = _starts([n_out * s * s for s in lengths])
    run = lambda lay, c, ml: _maps(lay, c, ml, H, d, scale, heads, weights, dtype)
    full = run(layer, cu.to(DEV), max(lengths))
    assert full.numel() == starts[-1]
    what = f'attn_maps d{d} {mode} B={B}'

    def part(a, b):
        c, lo, hi = _sub(cu, a, b)
        return run((layer[0][lo:hi], layer[1][lo:hi], False), c, max(lengths[a:b]))
    XS.assert_split_identity(full, starts, part, B, what)
    (qs, ks), cs = XS.sub_batch(layer[:2], cu, which)
    alone = run((qs, ks, False), cs.to(DEV), max(lengths[i] for i in which))
    XS.assert_picks_identity(full, starts, alone, which, what)
    cpu_layer = (qs.cpu(), ks.cpu(), False)
    w2 = None if weights is None else weights.reshape(1, -1)
    ref = [r[0] for r in MB.reference_maps([cpu_layer], cs, H, d, scale, heads, w2)]
    bound = [b[0] for b in MB.map_bound([cpu_layer], cs, H, d, scale, heads, w2, out_bf16=dtype == BF)]
    got = _blocks(alone.cpu(), _starts([r.numel() for r in ref]), [tuple(r.shape) for r in ref])
    XS.assert_inside(got, ref, bound, f'{what}, {len(which)} picks')


# ---------------------------------------------------------------------- A5

def test_attn_pool_bwd_70002_short_sequences():
    """The whole batch against float64 autograd, as test_attn_pool_gpu.test_pool_70002_short_sequences holds the forward; then dX of
    every sequence bit-equal inside the two sub-batches (the header: a sequence's dX does not depend on what it is packed with)."""
    from esme import _hip_attn_pool_bwd as HB
    E, H, C = 320, 20, 2
    lengths = XS.row_lengths()
    cu = XS.cu_of(lengths)
    B, T = len(lengths), sum(lengths)
    x = _randn((T, E), 600)
    U = _randn((C * H, E), 601, F32, 1.4426950408889634 / math.sqrt(E))
    d_out = _randn((B, C, E), 602)
    cud = cu.to(DEV)
    dx = torch.full((T, E), NAN, dtype=BF, device=DEV)
    got_dx, dU = HB.attn_pool_bwd(x, cud, U, d_out, H, C, dx=dx)
    assert got_dx is dx
    ref = PB.reference_pool_grads(x, cud, U, d_out, H)
    bound = PB.pool_bwd_bound(x, cud, U, d_out, H, ref[0], 'bf16')
    XS.assert_inside(dx, ref[0], bound[0], f'attn_pool_bwd dX B={B}')
    XS.assert_inside(dU, ref[1], bound[1], f'attn_pool_bwd dU B={B}')

    def part(a, b):
        c, lo, hi = _sub(cu, a, b)
        return HB.attn_pool_bwd(x[lo:hi], c, U, d_out[a:b], H, C, dx=torch.full((hi - lo, E), NAN, dtype=BF, device=DEV))[0]
    XS.assert_split_identity(dx, cu.tolist(), part, B, f'attn_pool_bwd dX B={B}')


@pytest.mark.parametrize('dtype', SB.DTYPES, ids=('bfloat16', 'float32'))
def test_segment_mean_bwd_70002_short_sequences(dtype):
    from esme import _hip_segment_mean_bwd as HS
    E = 320
    lengths = XS.row_lengths()
    dy, cu, T = SB.make_case(('many', dtype, E), device=DEV, lengths=lengths)
    assert dy.shape[0] == 70002 and T > 400000
    dx = torch.full((T, E), NAN, dtype=dtype, device=DEV)
    assert HS.segment_mean_bwd(dy, cu, T, d_x=dx) is dx
    assert SB.equal_bits(dx, SB.expected(dy, cu, T)), f'segment_mean_bwd {dtype} B=70 002: not the bits of the definition'


# ====================================================================== B. offsets past 2^31 inside and between sequences

class _Wide:
    """q, k, v, o, dO, dq, dk, dv as column blocks (128 columns apart: 16-byte aligned, never adjacent) of one (2166, 2^20) bfloat16
    buffer that is never filled: only the live columns are written or read."""

    def __init__(self, d):
        self.d, self.E, self.scale = d, d, d ** -0.5            # H = 1
        self.lengths, self.T = WIDE, sum(WIDE)
        self.cross = XS.crossing(WIDE, WIDE_LD)
        assert self.cross['inside'] == [(0, 2048)] and self.cross['sequences'] == [1, 2]
        self.cu = XS.cu_of(WIDE)
        self.buf = XS.wide_buffer(self.T, WIDE_LD, BF, DEV)
        names = ('q', 'k', 'v', 'o', 'do', 'dq', 'dk', 'dv')
        self.blk = {n: self.buf[:, 128 * i:128 * i + d] for i, n in enumerate(names)}
        for b in self.blk.values():
            assert b.stride(0) == WIDE_LD and b.data_ptr() % 16 == 0
        for i, n in enumerate(('q', 'k', 'v')):
            self.blk[n].copy_(_randn((self.T, d), 700 + d + i, scale=math.sqrt(1.5 if n != 'v' else 1.0)))
        self.blk['do'].copy_(_randn((self.T, d), 710 + d))
        for n in ('o', 'dq', 'dk', 'dv'):
            self.blk[n].fill_(NAN)

    def contiguous(self, *names):
        return tuple(self.blk[n].contiguous() for n in names)

    def cpu(self, *names):
        return tuple(self.blk[n].cpu() for n in names)

    def free(self):
        self.blk.clear()
        self.buf = None
        torch.cuda.empty_cache()


WIDE_DIMS = (32, 64)


@pytest.mark.parametrize('d', WIDE_DIMS)
def test_attn_varlen_bwd_offsets_past_2_31(d):
    from esme import _hip, _hip_attn_bwd as HB
    wb = _Wide(d)
    try:
        cud, ml = wb.cu.to(DEV), max(WIDE)
        q, k, v, do = wb.contiguous('q', 'k', 'v', 'do')
        o = _hip.attn_varlen(q, k, v, cud, ml, 1, softmax_scale=wb.scale)        # (the forward on contiguous operands: not what is under test)
        wb.blk['o'].copy_(o)
        b = wb.blk
        HB.attn_varlen_bwd(b['q'], b['k'], b['v'], b['o'], b['do'], cud, ml, 1, wb.scale, b['dq'], b['dk'], b['dv'])
        torch.cuda.synchronize()
        strided = torch.cat(wb.contiguous('dq', 'dk', 'dv'), 1)
        plain = _attn_bwd(q, k, v, o, do, cud, ml, 1, wb.scale)
        what = f'attn_varlen_bwd d{d}, row stride 2^20'
        XS.assert_rows_equal(strided, plain, f'{what} against contiguous operands')
        qc, kc, vc, oc, gc = (t.cpu() for t in (q, k, v, o, do))
        ref = AB.reference_bwd(qc, kc, vc, gc, wb.cu, 1, d, wb.scale)[:3]
        bound = AB.bwd_bound(qc, kc, vc, oc, gc, wb.cu, 1, d, wb.scale)
        for i, name in enumerate(('dq', 'dk', 'dv')):
            XS.assert_inside(strided[:, i * d:(i + 1) * d].cpu(), ref[i], bound[i], f'{what} {name}')
    finally:
        wb.free()


@pytest.mark.parametrize('d', WIDE_DIMS)
def test_contact_layer_offsets_past_2_31(d):
    wb = _Wide(d)
    try:
        cud, ml = wb.cu.to(DEV), max(WIDE)
        w = torch.tensor([[0.8], [-1.3]], device=DEV)
        b = wb.blk
        strided = _contacts([(b['q'], b['k'], False), (b['k'], b['v'], False)], cud, ml, 1, d, wb.scale, w)
        q, k, v = wb.contiguous('q', 'k', 'v')
        plain = _contacts([(q, k, False), (k, v, False)], cud, ml, 1, d, wb.scale, w)
        what = f'contact_layer d{d}, row stride 2^20'
        XS.assert_rows_equal(strided, plain, f'{what} against contiguous operands')
        layers = [(q.cpu(), k.cpu(), False), (k.cpu(), v.cpu(), False)]
        ref = CB.reference_contacts(layers, wb.cu, 1, d, wb.scale, w.cpu(), BIAS)
        bound = CB.contact_bound(layers, wb.cu, 1, d, wb.scale, w.cpu(), BIAS)
        got = _blocks(strided.cpu(), _starts([r.numel() for r in ref]), [tuple(r.shape) for r in ref])
        XS.assert_inside(got, ref, bound, what)
    finally:
        wb.free()


@pytest.mark.parametrize('d', WIDE_DIMS)
def test_contact_features_offsets_past_2_31(d):
    wb = _Wide(d)
    try:
        cud, ml = wb.cu.to(DEV), max(WIDE)
        pairs = FB.make_pairs(WIDE, seed=d)
        first = wb.cross['inside'][0][1] - 1                                        # kept row i is in-sequence row i + 1
        assert int(((pairs[:, 0] == 0) & ((pairs[:, 1] >= first) | (pairs[:, 2] >= first))).sum()) >= 3 and bool((pairs[:, 0] == 1).any())
        b = wb.blk
        strided = _features([(b['q'], b['k'], False), (b['k'], b['v'], False)], cud, ml, 1, d, wb.scale, pairs.to(DEV))
        q, k, v = wb.contiguous('q', 'k', 'v')
        plain = _features([(q, k, False), (k, v, False)], cud, ml, 1, d, wb.scale, pairs.to(DEV))
        what = f'contact_features d{d}, row stride 2^20'
        XS.assert_rows_equal(strided, plain, f'{what} against contiguous operands')
        layers = [(q.cpu(), k.cpu(), False), (k.cpu(), v.cpu(), False)]
        ref = FB.reference_features(layers, wb.cu, 1, d, wb.scale, pairs)
        bound = FB.feature_bound(layers, wb.cu, 1, d, wb.scale, pairs)
        XS.assert_inside(strided.cpu(), ref, bound, what)
    finally:
        wb.free()


@pytest.mark.parametrize('d', WIDE_DIMS)
def test_attn_maps_offsets_past_2_31(d):
    wb = _Wide(d)
    try:
        cud, ml = wb.cu.to(DEV), max(WIDE)
        b = wb.blk
        strided = _maps((b['q'], b['k'], False), cud, ml, 1, d, wb.scale, [0])
        q, k = wb.contiguous('q', 'k')
        plain = _maps((q, k, False), cud, ml, 1, d, wb.scale, [0])
        what = f'attn_maps d{d}, row stride 2^20'
        XS.assert_rows_equal(strided, plain, f'{what} against contiguous operands')
        layer = (q.cpu(), k.cpu(), False)
        ref = [r[0] for r in MB.reference_maps([layer], wb.cu, 1, d, wb.scale, [0])]
        bound = [x[0] for x in MB.map_bound([layer], wb.cu, 1, d, wb.scale, [0])]
        got = _blocks(strided.cpu(), _starts([r.numel() for r in ref]), [tuple(r.shape) for r in ref])
        XS.assert_inside(got, ref, bound, what)
    finally:
        wb.free()


# ====================================================================== C. offsets past 2^31: the row kernels

ROWS_M, ROWS_LD = 70000, 32768          # tests/test_gemm_wgrad_gpu.test_row_offsets_are_64_bit's buffer: row 65 536 starts at element 2^31


def test_embed_bwd_row_offsets_past_2_31():
    from esme import _hip_embed_bwd as HE
    V, E, m, p = 33, 64, 32, 1
    buf = XS.wide_buffer(ROWS_M, ROWS_LD, BF, DEV)
    try:
        dx = buf[:, 64:64 + E]
        dx.copy_(_randn((ROWS_M, E), 800))
        tok = EB.make_tokens(ROWS_M, V, 'skew', 801, m, p).to(DEV)
        assert bool(EB._valid(tok[65536:], V, m, p).any())                           # rows past element 2^31 count
        de = torch.full((V, E), EB.PREFILL, dtype=BF, device=DEV)
        assert HE.embed_bwd(dx, tok, V, m, p, d_table=de) is de
        plain = HE.embed_bwd(dx.contiguous(), tok, V, m, p, d_table=torch.full((V, E), EB.PREFILL, dtype=BF, device=DEV))
        XS.assert_rows_equal(de, plain, 'embed_bwd, row stride 32 768, against a contiguous d_x')
        XS.assert_inside(de, EB.reference(dx, tok, V, m, p), EB.bound(dx, tok, V, m, p)[0], f'embed_bwd T={ROWS_M}, row stride {ROWS_LD}')
    finally:
        del buf
        torch.cuda.empty_cache()


def test_segment_mean_bwd_row_offsets_past_2_31():
    """d_y (B rows) and d_x (T rows) as two column blocks of one canary-filled buffer, lengths from {0, 1, 2}: both B and T pass row
    65 536.  bfloat16: the float32 instance's buffer of this shape would be twice what a test here may hold."""
    from esme import _hip_segment_mean_bwd as HS
    E = 64
    lengths = np.random.Generator(np.random.PCG64(9)).integers(0, 3, size=68000).tolist()
    dy0, cu, T = SB.make_case(('wide', BF, E), device=DEV, lengths=lengths)
    B = len(lengths)
    assert 65536 < B <= ROWS_M and 65536 < T <= ROWS_M
    buf = XS.wide_buffer(ROWS_M, ROWS_LD, BF, DEV)
    try:
        buf.view(torch.int16).fill_(CANARY)
        dy, dx = buf[:B, 64:64 + E], buf[:T, 256:256 + E]
        dy.copy_(dy0)
        assert HS.segment_mean_bwd(dy, cu, T, d_x=dx) is dx
        torch.cuda.synchronize()
        assert SB.equal_bits(dx.contiguous(), SB.expected(dy0, cu, T)), 'segment_mean_bwd, row stride 32 768: not the bits of the definition'
        R = max(B, T)
        XS.assert_untouched(buf[:R], CANARY, (0, R), [(64, 64 + E), (256, 256 + E)], 'segment_mean_bwd')
        XS.assert_untouched(buf[R:], CANARY, (0, 0), [], 'segment_mean_bwd, rows behind the operands')
        bits = buf.view(torch.int16)
        assert bool((bits[B:R, 64:64 + E] == CANARY).all()) and bool((bits[T:R, 256:256 + E] == CANARY).all()), 'rows behind d_y or d_x were written'
        assert SB.equal_bits(dy.contiguous(), dy0), 'd_y changed'
    finally:
        del buf
        torch.cuda.empty_cache()


def test_attn_pool_bwd_row_offsets_past_2_31():
    """x and dx as column blocks; the last three sequences lie past row 65 536 (element 2^31).  Held over the whole batch, the tail
    sequences' ratio printed apart, as test_attn_pool_gpu.test_pool_embed_over_2_31_elements holds the forward's tail."""
    from esme import _hip_attn_pool_bwd as HB
    E, H, C = 64, 2, 1
    lengths = [66000, 2700, 300, 1]
    T = sum(lengths)
    cu = XS.cu_of(lengths)
    assert int(cu[1]) >= 65536 and T <= ROWS_M
    buf = XS.wide_buffer(ROWS_M, ROWS_LD, BF, DEV)
    try:
        x, dx = buf[:T, 64:64 + E], buf[:T, 256:256 + E]
        x.copy_(_randn((T, E), 810))
        dx.fill_(NAN)
        U = _randn((C * H, E), 811, F32, 1.4426950408889634 / math.sqrt(E))
        d_out = _randn((len(lengths), C, E), 812)
        cud = cu.to(DEV)
        got, dU = HB.attn_pool_bwd(x, cud, U, d_out, H, C, dx=dx)
        assert got is dx
        xc = x.contiguous()
        plain_dx, plain_dU = HB.attn_pool_bwd(xc, cud, U, d_out, H, C, dx=torch.full((T, E), NAN, dtype=BF, device=DEV))
        XS.assert_rows_equal(dx.contiguous(), plain_dx, 'attn_pool_bwd dX, row stride 32 768, against contiguous operands')
        XS.assert_rows_equal(dU, plain_dU, 'attn_pool_bwd dU, row stride 32 768, against contiguous operands')
        ref = PB.reference_pool_grads(xc, cud, U, d_out, H)
        bound = PB.pool_bwd_bound(xc, cud, U, d_out, H, ref[0], 'bf16')
        a = int(cu[1])
        XS.assert_inside(dx[a:], ref[0][a:], bound[0][a:], 'attn_pool_bwd dX, the three sequences past element 2^31')
        XS.assert_inside(dx, ref[0], bound[0], f'attn_pool_bwd dX T={T}, row stride {ROWS_LD}')
        XS.assert_inside(dU, ref[1], bound[1], f'attn_pool_bwd dU T={T}, row stride {ROWS_LD}')
    finally:
        del buf
        torch.cuda.empty_cache()


@pytest.mark.parametrize('bits', (4, 8))
def test_dequantize_t_row_offsets_past_2_31(bits):
    """out as a (K = 2112, N = 64) view with a row stride of 2^20 elements: rows 2048 .. 2111 start past element 2^31."""
    from esme import _hip, _hip_dequant_t as HT
    from esme.quantization import codebook_of
    K, N = 2112, 64
    w = _randn((N, K), 820 + bits, scale=0.05)
    if bits == 4:
        cb = codebook_of('nf4')
        codes, absmax = _hip.quantize_4bit(w, cb)
        run = lambda out: HT.dequantize_4bit_t(codes, absmax, cb, out=out)
    else:
        codes, scale = _hip.quantize_8bit(w)
        run = lambda out: HT.dequantize_8bit_t(codes, scale, out=out)
    want = run(None).contiguous()
    assert want.shape == (K, N) and bool(want[2048:].any())
    buf = XS.wide_buffer(K, WIDE_LD, BF, DEV)
    try:
        buf.view(torch.int16).fill_(CANARY)
        view = buf[:, 128:128 + N]
        assert run(view) is view
        torch.cuda.synchronize()
        XS.assert_rows_equal(view.contiguous(), want, f'dequantize_{bits}bit_t into a view with row stride 2^20 against the contiguous output')
        XS.assert_untouched(buf, CANARY, (0, K), [(128, 128 + N)], f'dequantize_{bits}bit_t', chunk=128)
    finally:
        del buf
        torch.cuda.empty_cache()


# ====================================================================== D. whole models, 70 000 peptides

def _peptide_batch(seed):
    from esme import synthetic as syn
    from test_extreme_shapes_gpu import peptides
    lengths = peptides()
    tokens, cu = syn.random_tokens(lengths, seed=seed), syn.cu_lens_of(lengths)
    which = XS.picks(len(lengths))
    sub_t, sub_cu = XS.sub_batch(tokens, cu, which)
    return lengths, tokens, cu, which, sub_t, sub_cu


def test_observers_more_than_65535_peptides():
    """predict_contacts, contact_features and attention_maps of a two-layer ESM2-8M over 70 000 peptides of 3 to 8 residues: B blocks of
    the right shapes, every one finite, the picks' blocks bit-equal to the picks run alone."""
    from esme import ContactHead
    from test_fullsize_gpu import load
    model, _, H = load('esm2_8m', L=2, seed=5)
    L = len(model.layers)
    head = ContactHead(L, H)
    head.regression.weight.data.copy_(torch.randn(1, L * H, generator=torch.Generator().manual_seed(9)))
    head.regression.bias.data.fill_(BIAS)
    model.set_contact_head(head)
    lengths, tokens, cu, which, sub_t, sub_cu = _peptide_batch(seed=16)
    B = len(lengths)
    td, cd, ml = tokens.to(DEV), cu.to(DEV), max(lengths)
    sd, scd, sml = sub_t.to(DEV), sub_cu.to(DEV), max(lengths[i] for i in which)
    flat = lambda blocks: torch.cat([b.reshape(-1) for b in blocks])

    got = model.predict_contacts(td, (cd, ml), logits=True)
    assert len(got) == B and all(tuple(g.shape) == (n - 2, n - 2) for g, n in zip(got, lengths)) and got[0].dtype == F32
    assert bool(torch.isfinite(flat(got)).all()), 'predict_contacts: non-finite logits'
    alone = model.predict_contacts(sd, (scd, sml), logits=True)
    XS.assert_rows_equal(flat([got[i] for i in which]), flat(alone), f'predict_contacts B={B}: the picks against the picks alone')
    del got

    X, pairs = model.contact_features(td, (cd, ml))
    assert X.shape == (sum((n - 2) * (n - 3) // 2 for n in lengths), L * H) and X.dtype == F32 and bool(torch.isfinite(X).all())
    assert set(pairs[:, 0].unique().tolist()) == {s for s, n in enumerate(lengths) if n >= 4}          # every sequence with a pair i < j
    Xa, pa = model.contact_features(sd, (scd, sml))
    lookup = torch.full((B,), -1, dtype=torch.int64, device=DEV)
    lookup[torch.tensor(which, device=DEV)] = torch.arange(len(which), device=DEV)
    sel = (lookup[pairs[:, 0].long()] >= 0).nonzero().reshape(-1)
    mine = pairs[sel].clone()
    mine[:, 0] = lookup[mine[:, 0].long()].to(mine.dtype)
    assert torch.equal(mine, pa), 'contact_features: the pair lists of the picks differ'
    XS.assert_rows_equal(X[sel], Xa, f'contact_features B={B}: the picks against the picks alone')
    del X

    maps = model.attention_maps(td, (cd, ml), layers=[-1], head_weights='mean', dtype=BF)
    assert len(maps) == B and all(tuple(m.shape) == (1, n, n) for m, n in zip(maps, lengths)) and maps[0].dtype == BF
    assert bool(torch.isfinite(flat(maps).float()).all()), 'attention_maps: non-finite entries'
    alone = model.attention_maps(sd, (scd, sml), layers=[-1], head_weights='mean', dtype=BF)
    XS.assert_rows_equal(flat([maps[i] for i in which]), flat(alone), f'attention_maps B={B}: the picks against the picks alone')


def _oracle_step():
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    spec = importlib.util.spec_from_file_location('make_golden_full_grad', os.path.join(golden, 'make_golden_full_grad.py'))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk


@pytest.mark.parametrize('kind', ('esm2', 'esmc'))
def test_training_step_more_than_65535_peptides(tmp_path, kind):
    """forward_trainable + cross_entropy + backward of the two tiny fixture models over 70 000 peptides.  The mask selects tokens of the
    picks only, so every other sequence contributes exact zeros and the truth is the oracle's float64 step
    (tests/golden/make_golden_full_grad.step) on the picks alone.  The bar per tensor, and of the loss, is the project's recipe: 2 x
    the relative Frobenius error of the same step in bfloat16 against that truth, computed here on the CPU."""
    import esme
    from esme import synthetic as syn
    from golden_util import load_golden, rel_fro
    from test_lora_gpu import tiny
    g13 = load_golden('g13_lora.npz')
    L, E, H, seed = (int(g13[f'{kind}_{k}']) for k in ('L', 'E', 'H', 'seed'))
    model = tiny(tmp_path, kind, L, E, H, seed).mark_trainable().train()
    lengths, tokens, cu, which, sub_t, sub_cu = _peptide_batch(seed=17)
    B = len(lengths)
    # a third of the picks' residues (never <cls> / <eos>) are masked; no token of any other sequence is
    rng = np.random.Generator(np.random.PCG64(18))
    cul = cu.tolist()
    mask = torch.zeros(tokens.numel(), dtype=torch.bool)
    for i in which:
        inner = np.arange(cul[i] + 1, cul[i + 1] - 1)
        mask[rng.choice(inner, size=max(1, len(inner) // 3), replace=False)] = True
    tokens_in = torch.where(mask, torch.full_like(tokens, model.alphabet.mask_idx), tokens)
    sub_in, _ = XS.sub_batch(tokens_in, cu, which)
    sub_mask, _ = XS.sub_batch(mask, cu, which)
    assert int(sub_mask.sum()) == int(mask.sum()) >= len(which)
    sml = max(lengths[i] for i in which)

    mk = _oracle_step()
    weights = syn.synthetic_state_dict(kind, L, E, seed)
    loss64, g64 = mk.step(weights, H, torch.float64, sub_in, sub_t, sub_mask, sub_cu, sml)
    loss16, g16 = mk.step(weights, H, torch.bfloat16, sub_in, sub_t, sub_mask, sub_cu, sml)
    bars = {k: 2 * mk.rel(g16[k], g64[k]) for k in g64}
    loss_bar = 2 * abs(float(loss16) - float(loss64)) / abs(float(loss64))

    model.zero_grad(set_to_none=True)
    logits = model.forward_trainable(tokens_in.to(DEV), (cu.to(DEV), max(lengths)))
    assert logits.shape == (tokens.numel(), model.vocab_size)
    loss = esme.cross_entropy(logits, tokens.to(DEV), mask.to(DEV), alphabet=model.alphabet)
    loss.backward()
    err = abs(float(loss) - float(loss64)) / abs(float(loss64))
    print(f'\n[extreme-train] {kind} B={B} loss {float(loss):.5f} (float64 on the picks {float(loss64):.5f}): error {err:.2e}, bar {loss_bar:.2e}')
    failures = [] if err <= loss_bar else [('loss', err, loss_bar)]
    seen = 0
    for name, p in model.named_parameters():
        if name not in g64:
            assert p.grad is None, name
            continue
        seen += 1
        assert p.grad is not None and bool(torch.isfinite(p.grad.float()).all()), name
        e = rel_fro(p.grad.float().cpu(), g64[name])
        print(f'[extreme-train] {kind} {name:44s} error {e:.4f}  bar {bars[name]:.4f}  ({e / bars[name]:.2f})')
        if e > bars[name]:
            failures.append((name, e, bars[name]))
    assert seen == len(g64)
    assert not failures, failures
