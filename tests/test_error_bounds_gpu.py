"""Every kernel entry point held to its per-element error bound against float64 (tests/error_bounds.py).

The float64 reference is formed on the GPU from the tensors actually handed to the kernel (bf16 / fp16 values, or hi + lo).
Each check returns its worst err / bound ratio; the ratios per kernel family and the rounding bias of every kernel whose last
step is a single rounding are printed at the end of the module (run with -s).  Bit-equality checks cover what the ABI promises
exactly: every esme_gemm_opts_t configuration, pair_to_f32, embed_positions, the fp32 stream's bf16 operand.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import error_bounds as eb
import gemm_operands as ops
from gemm_operands import BF, BIAS_MIN_ELEMENTS, DEV, H16, rnd
from oracle import esm_oracle as O
from esme import _hip
from esme import synthetic as syn

pytestmark = pytest.mark.gpu
LOG2E = 1.4426950408889634
LEDGER = ops.Ledger('error bounds')
record, record_bias = LEDGER.record, LEDGER.record_bias
# `persist` below: under 2 * (compute units & ~7) tiles of 256 x 256 (512 on an MI355X; the largest GEMM here has 85) option 1 runs the
# per-tile kernel, the same launch as option 0 (tests/gemm_path.py); the persistent kernel is held to these bounds in
# tests/test_gemm_persistent_bounds_gpu.py.


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    LEDGER.report()


def cu_of(lengths):
    return syn.cu_lens_of(lengths).to(DEV)


# ------------------------------------------------------------------ GEMM

GEMM_SHAPES = [(1, 320, 64), (255, 33, 5120), (257, 1280, 64), (4099, 384, 5120), (1000, 1280, 640)]


@pytest.mark.parametrize('M,N,K', GEMM_SHAPES)
@pytest.mark.parametrize('tile', [1, 2])
@pytest.mark.parametrize('persist', [0, 1])
def test_gemm_plain_epilogues(M, N, K, tile, persist):
    a, w, b, r = ops.plain_operands(M, N, K)
    lay = eb.gemm_layout(128 * tile, 128 * tile)
    with _hip.gemm_options(tile=tile, persist=persist):
        for epi, bias in (('none', b), ('none', None), ('gelu', b), ('residual', b)):
            code = {'none': _hip.EPI_NONE, 'gelu': _hip.EPI_GELU, 'residual': _hip.EPI_RESIDUAL}[epi]
            got = _hip.gemm(a, w, bias, code, resid=r if epi == 'residual' else None, alpha=0.75)
            ref, bound, pre = eb.gemm_reference(a, w, bias, epi, resid=r, alpha=0.75)
            what = f'gemm {epi}{"" if bias is not None else " nobias"} {M}x{N}x{K} tile{tile} persist{persist}'
            record(f'gemm bf16 {epi}', eb.assert_bounded(got, ref, bound, what, lay), eb.budget_used(got, ref, bound, pre))
            if got.numel() >= BIAS_MIN_ELEMENTS:
                record_bias(f'gemm bf16 {epi}', got, ref, pre, 'bf16')
        if N % 64 == 0:
            F = N // 2
            wa, wf = w[:F], w[F:]
            packed = ops.swiglu_pack(wa, wf)
            got = _hip.gemm(a, packed, None, _hip.EPI_SWIGLU)
            ref, bound, pre = eb.swiglu_reference(a, wa, wf)
            record('gemm bf16 swiglu', eb.assert_bounded(got, ref, bound, f'gemm swiglu {M}x{N}x{K} tile{tile} persist{persist}', lay),
                   eb.budget_used(got, ref, bound, pre))
            if got.numel() >= BIAS_MIN_ELEMENTS:
                record_bias('gemm bf16 swiglu', got, ref, pre, 'bf16')


@pytest.mark.parametrize('kind', ['plain', 'dc20', 'outlier'])
@pytest.mark.parametrize('tile', [1, 2])
@pytest.mark.parametrize('persist', [0, 1])
def test_gemm_layernorm_fold(kind, tile, persist):
    T, E, N = 1000, 640, 1280
    x, wp, c1, c2 = ops.ln_fold_operands(T, E, N, 5 + len(kind), kind)
    sums = _hip.row_sums(x)
    with _hip.gemm_options(tile=tile, persist=persist):
        got = _hip.gemm_fused(x, wp, None, ln=(sums, E, 1e-5, c1, c2))
        gel = _hip.gemm_fused(x, wp, None, _hip.EPI_GELU, ln=(sums, E, 1e-5, c1, c2))
    y, pre = eb.ln_fold_reference(x, wp, c1, c2, 1e-5, sums)
    record('gemm LN fold', eb.assert_bounded(got, y, pre + eb.out_round(y, pre, 'bf16'), f'LN fold {kind} tile{tile} persist{persist}',
                                             eb.gemm_layout(128 * tile, 128 * tile)), eb.budget_used(got, y, pre + eb.out_round(y, pre, 'bf16'), pre))
    record_bias('gemm LN fold', got, y, pre, 'bf16')
    gp = eb.gelu_bound(y, pre, 5)                                      # the LN-folded site runs the degree-5 polynomial (gemm.hip:895, gemm_bf16_kernel)
    gv = eb.gelu64(y)
    record('gemm LN fold + gelu', eb.assert_bounded(gel, gv, gp + eb.out_round(gv, gp, 'bf16'), f'LN fold gelu {kind}'))


@pytest.mark.parametrize('d,H', [(16, 20), (32, 20), (64, 8)])
@pytest.mark.parametrize('q_scale', [0.0, 0.125 * LOG2E])
@pytest.mark.parametrize('tile', [1, 2])
@pytest.mark.parametrize('persist', [0, 1])
def test_gemm_fused_rotary(d, H, q_scale, tile, persist):
    lengths = [1, 63, 64, 65, 700]
    T, E = sum(lengths), H * d
    K = 320
    cu = cu_of(lengths)
    a, w, b = rnd((T, K), 50 + d), rnd((3 * E, K), 51 + d, 1 / math.sqrt(K)), rnd((3 * E,), 52, 0.1)
    cos, sin = O.rotary_tables(max(lengths), d, BF)
    cos, sin = cos.to(DEV), sin.to(DEV)
    pos, _ = _hip.seq_positions(cu, T)
    qs = q_scale if q_scale else None
    with _hip.gemm_options(tile=tile, persist=persist):
        got = _hip.gemm_fused(a, w, b, rot=(cos, sin, pos, d, 2 * E), q_scale=q_scale)
    y, _, pre = eb.gemm_reference(a, w, b)
    ref, bound = y.clone(), pre.clone()
    for blk in range(2):
        cs = slice(blk * E, (blk + 1) * E)
        r_, e_ = eb.rotary_bound(y[:, cs].reshape(T, H, d), pre[:, cs].reshape(T, H, d), cos, sin, pos,
                                 qs if blk == 0 else None)
        ref[:, cs], bound[:, cs] = r_.reshape(T, E), e_.reshape(T, E)
    record_bias('gemm fused rotary', got, ref, bound, 'bf16')
    pre = bound
    bound = bound + eb.out_round(ref, bound, 'bf16')
    record('gemm fused rotary' + (' + q_scale' if qs else ''),
           eb.assert_bounded(got, ref, bound, f'fused rotary d{d} q_scale {q_scale} tile{tile} persist{persist}'), eb.budget_used(got, ref, bound, pre))


@pytest.mark.parametrize('M,N,K', [(257, 1280, 640), (4099, 384, 5120)])
@pytest.mark.parametrize('tile', [1, 2])
@pytest.mark.parametrize('persist', [0, 1])
def test_gemm_residual_stats_and_fp32_stream(M, N, K, tile, persist):
    a, w, b, r, x32 = ops.residual_stream_operands(M, N, K)
    with _hip.gemm_options(tile=tile, persist=persist):
        nblk = _hip.stats_blocks(M, N)
        stats = torch.empty(nblk, M, 2, dtype=torch.float32, device=DEV)
        got = _hip.gemm_fused(a, w, b, _hip.EPI_RESIDUAL, resid=r, alpha=0.5, stats_out=stats)
        xs = x32.clone()
        x16 = _hip.gemm_fused(a, w, b, _hip.EPI_RESIDUAL, None, 0.5, resid32=xs)
    ref, bound, _ = eb.gemm_reference(a, w, b, 'residual', resid=r, alpha=0.5)
    record('gemm bf16 residual', eb.assert_bounded(got, ref, bound, f'residual {M}x{N}x{K} tile{tile} persist{persist}'))
    # stats_out: per row {sum, sum of squares} of the ROUNDED outputs, fp32 partials per column block
    s_ref, sb = ops.stats_reference(got, nblk)
    st = stats.double().sum(0)
    record('gemm stats_out', eb.assert_bounded(st, s_ref, sb, 'stats_out'))
    # fp32 residual stream: x32 <- fma(alpha, acc + bias, x32) (gemm.hip:952, gemm_bf16_kernel), one rounding; x16 = its bf16 rounding, bit for bit
    y, _, pre = eb.gemm_reference(a, w, b)
    ref32 = x32.double() + 0.5 * y
    pre32 = 0.5 * pre + eb.U32 * ref32.abs()
    record('gemm resid32', eb.assert_bounded(xs, ref32, pre32, 'resid32 stream'))
    assert torch.equal(x16, xs.to(BF))


@pytest.mark.parametrize('M,N,K', [(255, 384, 320), (4099, 1280, 640)])
@pytest.mark.parametrize('tile', [1, 2])
@pytest.mark.parametrize('persist', [0, 1])
def test_gemm_f16(M, N, K, tile, persist):
    """Precision 'half': fp16 operands and output; the pair stream (scaled, with the extension K-tile)."""
    a, w, b = ops.f16_operands(M, N, K)
    with _hip.gemm_options(tile=tile, persist=persist):
        got = _hip.gemm_fused(a, w, b)
        gel = _hip.gemm_fused(a, w, b, _hip.EPI_GELU)
        # pair stream: x = (hi + lo) * scale_in; x + 0.7 (acc + b), stored * scale_out as an fp16 pair; ext tile of 3 columns
        g = torch.Generator().manual_seed(73)
        x = (torch.randn(M, N, generator=g) * 3).to(DEV)
        si = (0.75 + 0.5 * torch.rand(N, generator=g)).to(DEV)
        so = (0.75 + 0.5 * torch.rand(N, generator=g)).to(DEV)
        sel = torch.tensor([3, 100, N - 1], dtype=torch.int32, device=DEV)
        hi = x.to(H16)
        lo = (x - hi.float()).to(H16)
        pair = torch.zeros(M, 2 * N + 64, dtype=H16, device=DEV)
        pair[:, :N], pair[:, N + 64:] = hi, lo
        xin = (hi.double() + lo.double()) * si.double()
        _hip.gemm_fused(a, w, b, _hip.EPI_RESIDUAL, None, 0.7, resid_pair=pair, pair_scale=(si, so), pair_ext=sel)
    ref, bound, pre = eb.gemm_reference(a, w, b, out_fmt='fp16')
    record('gemm fp16 none', eb.assert_bounded(got, ref, bound, f'f16 {M}x{N}x{K} tile{tile} persist{persist}'), eb.budget_used(got, ref, bound, pre))
    if got.numel() >= BIAS_MIN_ELEMENTS:
        record_bias('gemm fp16 none', got, ref, pre, 'fp16')
    gv = eb.gelu64(ref)
    gp = eb.gelu_bound(ref, pre, 7)
    record('gemm fp16 gelu', eb.assert_bounded(gel, gv, gp + eb.out_round(gv, gp, 'fp16'), 'f16 gelu'))
    # (gemm.hip:788-789, gemm_bf16_kernel): x * si one product, fma with alpha, then * so one product; the pair split of the stored value
    xn = xin + 0.7 * ref
    pre_x = eb.U32 * xin.abs() + 0.7 * pre + eb.U32 * xn.abs()
    st_ref = xn * so.double()
    st_pre = pre_x * so.double() + eb.U32 * st_ref.abs()
    got_st = pair[:, :N].double() + pair[:, N + 64:].double()
    record('gemm fp16 pair stream', eb.assert_bounded(got_st, st_ref, st_pre + eb.out_round(st_ref, st_pre, 'fp16', pair=True),
                                                      'f16 pair stream'))
    assert torch.equal(pair[:, N:N + 3], pair[:, N + 64:][:, sel.long()])       # the extension tile holds lo of the selected columns
    assert not bool(pair[:, N + 3:N + 64].any())


@pytest.mark.parametrize('form', ['single', 'single_q_scale', 'qk_pair'])
@pytest.mark.parametrize('tile', [1, 2])
@pytest.mark.parametrize('persist', [0, 1])
def test_gemm_f16_ln_fold_extension_tile_and_rotary(form, tile, persist):
    """Precision 'half' QKV projection: the fp16 pair stream [hi | ext | lo] with 3 massive channels, A = [hi | ext] over K = E + 64
    against W = [W' | W'[:, sel] | 0], LayerNorm folded, rotary in the epilogue (fp16 tables; the q/k pair output: fp32 tables),
    q_scale, the plan guard's qk_sumsq."""
    H, d, lengths = 8, 64, [1, 63, 64, 65, 700]
    T, E = sum(lengths), H * d
    cu = cu_of(lengths)
    pos, _ = _hip.seq_positions(cu, T)
    sel = torch.tensor([5, 77, 300], dtype=torch.int32)
    x32, _, wext, c1, c2 = (t.to(DEV) for t in ops.f16_ln_fold_operands(T, E, 3 * E, 90 + len(form), sel))
    pair = torch.zeros(T, 2 * E + 64, dtype=H16, device=DEV)
    sums = torch.empty(1, T, 2, dtype=torch.float32, device=DEV)
    _hip.stream_operand(x32, pair, sums, pair=True, ext_sel=sel.to(DEV))
    A = pair[:, :E + 64]
    qs = 0.125 * LOG2E if form == 'single_q_scale' else 0.0
    sumsq = torch.zeros(2, H, dtype=torch.int32, device=DEV)
    tdt = torch.float32 if form == 'qk_pair' else H16
    cos, sin = (t.to(tdt).to(DEV) for t in O.rotary_tables(max(lengths), d, torch.float32))
    with _hip.gemm_options(tile=tile, persist=persist):
        if form == 'qk_pair':
            got = _hip.gemm_fused(A, wext, None, ln=(sums, E, 1e-5, c1, c2), rot=(cos, sin, pos, d, 2 * E), pair_out=True, pair_cols=2 * E)
        else:
            got = _hip.gemm_fused(A, wext, None, ln=(sums, E, 1e-5, c1, c2), rot=(cos, sin, pos, d, 2 * E), q_scale=qs, qk_sumsq=sumsq)
    y, pre = eb.ln_fold_reference(A, wext, c1, c2, 1e-5, sums, dim=E)
    ref, bound = y.clone(), pre.clone()
    for blk in range(2):
        cs = slice(blk * E, (blk + 1) * E)
        r_, e_ = eb.rotary_bound(y[:, cs].reshape(T, H, d), pre[:, cs].reshape(T, H, d), cos, sin, pos, qs if (blk == 0 and qs) else None)
        ref[:, cs], bound[:, cs] = r_.reshape(T, E), e_.reshape(T, E)
    what = f'f16 LN fold + ext + rotary {form} tile{tile} persist{persist}'
    if form == 'qk_pair':
        qk = got[:, :2 * E].double() + got[:, 3 * E:].double()
        record('gemm fp16 LN fold qk pair', eb.assert_bounded(qk, ref[:, :2 * E], bound[:, :2 * E] + eb.out_round(ref[:, :2 * E], bound[:, :2 * E], 'fp16', pair=True), what))
        vv = got[:, 2 * E:3 * E]
        record('gemm fp16 LN fold', eb.assert_bounded(vv, ref[:, 2 * E:], bound[:, 2 * E:] + eb.out_round(ref[:, 2 * E:], bound[:, 2 * E:], 'fp16'), what + ' v'))
        return
    record('gemm fp16 LN fold' + (' + q_scale' if qs else ''), eb.assert_bounded(got, ref, bound + eb.out_round(ref, bound, 'fp16'), what))
    record_bias('gemm fp16 LN fold', got, ref, bound, 'fp16')
    # the plan guard: max over rows of the stored q / k row norms per head (fp32 sums of d exact squares)
    st = got[:, :2 * E].double().view(T, 2, H, d)
    nrm = (st * st).sum(-1).amax(0)
    gs = sumsq.view(torch.float32).double()
    assert bool(((gs - nrm).abs() <= eb.C_DOT * eb.U32 * math.sqrt(d) * nrm + eb.U32 * nrm).all()), (gs, nrm)


@pytest.mark.parametrize('M,N,K', [(257, 384, 256), (45000, 512, 256)])
@pytest.mark.parametrize('tile', [1, 2])
@pytest.mark.parametrize('persist', [0, 1])
def test_gemm_split_operand_pair(M, N, K, tile, persist):
    """'exact' mode: A = [hi | lo] over the doubled K, result as a bf16 pair, GELU pair, fp32 c32."""
    g = torch.Generator().manual_seed(M + N)
    x = (torch.randn(M, K, generator=g) * 3.0).to(DEV)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(BF).to(DEV)
    b = torch.randn(N, generator=g).to(BF).to(DEV)
    hi = x.to(BF)
    a = torch.cat((hi, (x - hi.float()).to(BF)), 1).contiguous()
    w2 = torch.cat((w, w), 1)
    with _hip.gemm_options(tile=tile, persist=persist):
        out = _hip.gemm_fused(a, w, b, split_a=True, pair_out=True)
        outg = _hip.gemm_fused(a, w, b, _hip.EPI_GELU, split_a=True, pair_out=True)
        y32 = torch.empty(M, N, dtype=torch.float32, device=DEV)
        _hip.gemm_fused(a, w, b, split_a=True, out32=y32)
    ref, bound, ppre = eb.gemm_reference(a, w2, b, pair=True)
    join = out[:, :N].double() + out[:, N:].double()
    record('gemm split pair', eb.assert_bounded(join, ref, bound, f'split pair {M}x{N}x{K} tile{tile} persist{persist}', eb.gemm_layout()),
           eb.budget_used(join, ref, bound, ppre))
    gref, gbound, _ = eb.gemm_reference(a, w2, b, 'gelu', pair=True)
    record('gemm split pair gelu', eb.assert_bounded(outg[:, :N].double() + outg[:, N:].double(), gref, gbound, 'split pair gelu'))
    _, _, pre = eb.gemm_reference(a, w2, b)
    record('gemm split c32', eb.assert_bounded(y32, ref, pre + eb.out_round(ref, pre, 'fp32'), 'split c32'))


# ------------------------------------------------------------------ GEMM: every esme_gemm_opts_t configuration, same bits

RASTERS = [(0, 0), (1, 1), (3, 4), (5, 7), (64, 1), (2, 64)]


@pytest.mark.parametrize('family', ['none', 'gelu', 'residual_stats', 'swiglu', 'ln_fold', 'rotary'])
def test_gemm_options_bit_equal(family):
    """tile x raster (gm, gn) x persist: groups that do not divide tiles_m / tiles_n (M = 1000: 8 / 4 row tiles; N = 1280: 10 / 5
    column tiles) and gm > tiles_m (64) -- every configuration the same bits, stats_out too (within a tile size, whose stats_out
    layout differs).  Under 2 * (compute units & ~7) tiles option persist=1 runs the per-tile kernel (tests/gemm_path.py), so at this shape
    both options are the same launch; the persistent kernel runs these rasters in tests/test_gemm_persistent_bounds_gpu.py."""
    M, N, K = 1000, 1280, 640
    a, w, b = rnd((M, K), 80), rnd((N, K), 81, 1 / math.sqrt(K)), rnd((N,), 82, 0.5)
    r = rnd((M, N), 83)
    outs, stats = {}, {}
    if family == 'ln_fold':
        x, wp, c1, c2 = ops.ln_fold_operands(M, K, N, 84, 'plain')
        sums = _hip.row_sums(x)
    if family == 'rotary':
        lengths = [1, 300, 64, 635]
        cos, sin = O.rotary_tables(max(lengths), 64, BF)
        cos, sin = cos.to(DEV), sin.to(DEV)
        pos, _ = _hip.seq_positions(cu_of(lengths), M)
    for tile in (1, 2):
        for gm, gn in RASTERS:
            for persist in (0, 1):
                key = (tile, gm, gn, persist)
                with _hip.gemm_options(tile=tile, raster=(gm, gn), persist=persist):
                    if family == 'none':
                        outs[key] = _hip.gemm(a, w, b)
                    elif family == 'gelu':
                        outs[key] = _hip.gemm(a, w, b, _hip.EPI_GELU)
                    elif family == 'residual_stats':
                        st = torch.full((_hip.stats_blocks(M, N), M, 2), float('nan'), device=DEV)
                        outs[key] = _hip.gemm_fused(a, w, b, _hip.EPI_RESIDUAL, resid=r, alpha=0.5, stats_out=st)
                        stats[key] = st
                    elif family == 'swiglu':
                        outs[key] = _hip.gemm(a, w, None, _hip.EPI_SWIGLU)
                    elif family == 'ln_fold':
                        outs[key] = _hip.gemm_fused(x, wp, None, ln=(sums, K, 1e-5, c1, c2))
                    else:
                        outs[key] = _hip.gemm_fused(a, w, b, rot=(cos, sin, pos, 64, 2 * 384))
    base = outs[(1, 0, 0, 0)]
    for key, o in outs.items():
        assert torch.equal(o, base), f'{family}: configuration (tile, gm, gn, persist) = {key} differs from the default'
    for key, st in stats.items():
        assert bool(torch.isfinite(st).all()), f'stats_out {key}: a block was not written'
        ref = stats[(key[0], 0, 0, 0)]
        assert torch.equal(st, ref), f'stats_out configuration {key} differs'


# ------------------------------------------------------------------ attention

LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 700, 1253]


def _qkv(T, E, seed, dtype, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(T, E, generator=g) * scale).to(dtype).to(DEV) for _ in range(3)]


ATTN_BF16 = [  # (d, H, variant, spec, q_blocks)
    (16, 8, 0, 1, 0), (32, 8, 0, 1, 0), (64, 4, 0, 1, 0), (128, 2, 0, 1, 0),
    (64, 4, 1, 0, 1), (64, 4, 1, 0, 2), (32, 8, 1, 0, 0), (128, 2, 1, 0, 0), (16, 8, 1, 0, 0),
    (64, 4, 4, 1, 0), (64, 4, 4, 0, 0), (64, 4, 8, 1, 0), (64, 4, 8, 0, 0),
    (64, 4, 2, 1, 0), (32, 8, 2, 1, 0),
]


@pytest.mark.parametrize('d,H,variant,spec,qb', ATTN_BF16)
def test_attention_bf16(d, H, variant, spec, qb):
    T, E = sum(LENGTHS), H * d
    cu = cu_of(LENGTHS)
    q, k, v = _qkv(T, E, d + variant, BF, 1.5)
    with _hip.attn_options(variant=variant, spec=spec, q_blocks=qb):
        got = _hip.attn_varlen(q, k, v, cu, max(LENGTHS), H)
    ref, bound, pre = eb.attention_reference(q, k, v, cu, H, d ** -0.5, 'bf16', 'bf16')
    record('attention bf16', eb.assert_bounded(got, ref, bound, f'attention bf16 d{d} variant {variant} spec {spec} qb {qb}',
                                               eb.attn_layout(cu, H, d)), eb.budget_used(got, ref, bound, pre))


@pytest.mark.parametrize('d,H', [(16, 8), (32, 8), (64, 4), (128, 2)])
def test_attention_bf16_exact_entry(d, H):
    T, E = sum(LENGTHS), H * d
    cu = cu_of(LENGTHS)
    q, k, v = _qkv(T, E, 3 * d, BF, 1.5)
    got = _hip.attn_varlen(q, k, v, cu, max(LENGTHS), H, exact=True)
    ref, bound, pre = eb.attention_reference(q, k, v, cu, H, d ** -0.5, 'bf16', 'bf16')
    record('attention bf16 exact', eb.assert_bounded(got, ref, bound, f'attention exact d{d}', eb.attn_layout(cu, H, d)), eb.budget_used(got, ref, bound, pre))


@pytest.mark.parametrize('d,H,variant', [(64, 4, 0), (64, 4, 4), (64, 4, 8), (32, 8, 0), (64, 4, 2)])
def test_attention_bf16_prescaled(d, H, variant):
    T, E = sum(LENGTHS), H * d
    cu = cu_of(LENGTHS)
    q, k, v = _qkv(T, E, 5 * d + variant, BF, 1.5)
    qs = (q.float() * (d ** -0.5 * LOG2E)).to(BF)
    with _hip.attn_options(variant=variant):
        got = _hip.attn_varlen(qs, k, v, cu, max(LENGTHS), H, q_prescaled=True)
    ref, bound, pre = eb.attention_reference(qs, k, v, cu, H, 1.0, 'bf16', 'bf16', log2_units=True)
    record('attention bf16 prescaled', eb.assert_bounded(got, ref, bound, f'attention prescaled d{d} variant {variant}',
                                                         eb.attn_layout(cu, H, d)), eb.budget_used(got, ref, bound, pre))


@pytest.mark.parametrize('d,H,form', [(d, H, f) for d, H in ((16, 8), (32, 8), (64, 4), (128, 2)) for f in ('default', 'exact', 'prescaled')
                                         if f != 'prescaled' or d in (32, 64)])     # (the fixed-reference form: the ping-pong kernel, d 32 / 64)
def test_attention_f16(d, H, form):
    T, E = sum(LENGTHS), H * d
    cu = cu_of(LENGTHS)
    q, k, v = _qkv(T, E, 7 * d + len(form), H16)
    if form == 'prescaled':
        q = (q.float() * (d ** -0.5 * LOG2E)).to(H16)
        got = _hip.attn_varlen(q, k, v, cu, max(LENGTHS), H, q_prescaled=True)
        ref, bound, pre = eb.attention_reference(q, k, v, cu, H, 1.0, 'fp16', 'fp16', log2_units=True, fixed_ref=4.0)
    else:
        got = _hip.attn_varlen(q, k, v, cu, max(LENGTHS), H, exact=form == 'exact')
        ref, bound, pre = eb.attention_reference(q, k, v, cu, H, d ** -0.5, 'fp16', 'fp16')
    lay = eb.attn_layout(cu, H, d, eb.FIXED_REF_ITEM_ROWS if form == 'prescaled' else 64)
    record(f'attention fp16 {form}', eb.assert_bounded(got, ref, bound, f'attention f16 {form} d{d}', lay), eb.budget_used(got, ref, bound, pre))
    # (no rounding-bias check for attention: the P rounding alone puts every element's pre-rounding bound near an ulp of o, far above
    # the 0.05-ulp filter, so no element would qualify)


@pytest.mark.parametrize('case', ['overflow', 'vanished'])
def test_attention_f16_redo_items(case):
    """Work items redone with exact maxima (P would leave fp16's range / every row sum vanishes) meet the same bound as the rest."""
    H, d, lengths = 4, 64, [300, 77, 513, 1, 65]
    T, E = sum(lengths), H * d
    cu = cu_of(lengths)
    g = torch.Generator().manual_seed(5)
    if case == 'overflow':
        q = (torch.randn(T, E, generator=g) * 4.0).to(H16)
        k = (torch.randn(T, E, generator=g) * 4.0).to(H16)
    else:
        q, k = torch.randn(T, E, generator=g), torch.randn(T, E, generator=g)
        k[:, ::d] = 4.0
        q[:, ::d] = -12.0 / 4.0 * math.sqrt(d)
        q, k = q.to(H16), k.to(H16)
    v = torch.randn(T, E, generator=g).to(H16).to(DEV)
    qs = (q.float() * (d ** -0.5 * LOG2E)).to(H16).to(DEV)
    k = k.to(DEV)
    got = _hip.attn_varlen(qs, k, v, cu, max(lengths), H, q_prescaled=True)
    if case == 'vanished':              # the batch does what it is for: rows whose sum at reference 4 is far under S * 2^-14 (attn.hip:1069-1076, attn_pp64_kernel)
        cl = cu.tolist()
        for s0, s1 in zip(cl[:-1], cl[1:]):
            t = qs[s0:s1].double().view(-1, H, d).transpose(0, 1) @ k[s0:s1].double().view(-1, H, d).permute(1, 2, 0)
            assert bool((torch.exp2(t - 4.0).sum(-1) < 0.5 * (s1 - s0) * 2.0 ** -14).any()), (s0, s1)
    ref, bound, pre = eb.attention_reference(qs, k, v, cu, H, 1.0, 'fp16', 'fp16', log2_units=True, fixed_ref=4.0)
    record('attention fp16 redo', eb.assert_bounded(got, ref, bound, f'attention f16 redo {case}', eb.attn_layout(cu, H, d, eb.FIXED_REF_ITEM_ROWS)),
           eb.budget_used(got, ref, bound, pre))
    gd = _hip.attn_varlen(q.to(DEV), k, v, cu, max(lengths), H)                # the default fp16 form on the same scores
    ref, bound, pre = eb.attention_reference(q.to(DEV), k, v, cu, H, d ** -0.5, 'fp16', 'fp16')
    record('attention fp16 redo', eb.assert_bounded(gd, ref, bound, f'attention f16 default {case}', eb.attn_layout(cu, H, d)), eb.budget_used(gd, ref, bound, pre))


@pytest.mark.parametrize('d,H', [(16, 8), (32, 8), (64, 4), (128, 2)])
def test_attention_split(d, H):
    T, E = sum(LENGTHS), H * d
    cu = cu_of(LENGTHS)
    g = torch.Generator().manual_seed(d)
    qkv = (torch.randn(T, 3 * E, generator=g) * 1.5).to(DEV)
    hi = qkv.to(BF)
    pair = torch.cat((hi, (qkv - hi.float()).to(BF)), 1).contiguous()
    x = pair[:, :3 * E].double() + pair[:, 3 * E:].double()
    out = _hip.attn_varlen_split(pair, cu, max(LENGTHS), H, d, d ** -0.5)
    got = out[:, :E].double() + out[:, E:].double()
    ref, bound, pre = eb.attention_reference(x[:, :E], x[:, E:2 * E], x[:, 2 * E:], cu, H, d ** -0.5, 'bf16pair', 'bf16', pair_out=True,
                                        qk_drop=2.0 ** -16)
    record('attention split', eb.assert_bounded(got, ref, bound, f'attention split d{d}', eb.attn_layout(cu, H, d)), eb.budget_used(got, ref, bound, pre))


@pytest.mark.parametrize('d,H,variant', [(16, 8, 0), (16, 8, 1), (32, 8, 0), (32, 8, 1), (32, 8, 2), (64, 4, 0), (64, 4, 1), (64, 4, 2)])
def test_attention_qkpair_f16(d, H, variant):
    T, E = sum(LENGTHS), H * d
    cu = cu_of(LENGTHS)
    g = torch.Generator().manual_seed(9 * d + variant)
    qk = torch.randn(T, 2 * E, generator=g) * 3.0
    hi = qk.to(H16)
    lo = (qk - hi.float()).to(H16)
    v = torch.randn(T, E, generator=g).to(H16)
    qkv = torch.cat((hi, v, lo), 1).contiguous().to(DEV)
    with _hip.attn_options(variant=variant):
        got = _hip.attn_varlen_qkpair(qkv, cu, max(LENGTHS), H, d, d ** -0.5)
    q = qkv[:, :E].double() + qkv[:, 3 * E:4 * E].double()
    k = qkv[:, E:2 * E].double() + qkv[:, 4 * E:].double()
    ref, bound, pre = eb.attention_reference(q, k, qkv[:, 2 * E:3 * E], cu, H, d ** -0.5, 'fp16', 'fp16', qk_drop=2.0 ** -22)
    record('attention qkpair fp16', eb.assert_bounded(got, ref, bound, f'attention qkpair d{d} variant {variant}', eb.attn_layout(cu, H, d)), eb.budget_used(got, ref, bound, pre))


# ------------------------------------------------------------------ row ops

def _ln_params(E, seed, bias=True):
    g = torch.Generator().manual_seed(seed)
    w = (1 + 0.1 * torch.randn(E, generator=g)).to(BF).to(DEV)
    b = (0.1 * torch.randn(E, generator=g)).to(BF).to(DEV) if bias else None
    return w, b


@pytest.mark.parametrize('T,E', [(1, 64), (1001, 1280), (37, 5120)])
@pytest.mark.parametrize('kind', ['plain', 'dc20'])
def test_layernorm_forms(T, E, kind):
    off = 20.0 if kind == 'dc20' else 0.5
    x = rnd((T, E), T + E, 2.0, offset=off)
    w, b = _ln_params(E, E)
    ref, bound, pre = eb.layernorm_reference(x, w, b, 1e-5, 'bf16')
    got = _hip.layernorm(x, w, b)
    record('layernorm bf16', eb.assert_bounded(got, ref, bound, f'layernorm {T}x{E} {kind}'), eb.budget_used(got, ref, bound, pre))
    if got.numel() >= 10 ** 6:                                         # (the 1001 x 1280 shape)
        record_bias('layernorm bf16', got, ref, pre, 'bf16')
    # strided in place inside a (T, 3E) buffer
    buf = torch.zeros(T, 3 * E, dtype=BF, device=DEV)
    buf[:, E:2 * E] = x
    _hip.layernorm(buf[:, E:2 * E], w, b, out=buf[:, E:2 * E])
    record('layernorm bf16', eb.assert_bounded(buf[:, E:2 * E], ref, bound, 'layernorm strided in place'))
    assert not bool(buf[:, :E].any()) and not bool(buf[:, 2 * E:].any())
    # fp32 input (layernorm_f32): x32 exact values
    x32 = (torch.randn(T, E, generator=torch.Generator().manual_seed(3)) * 2 + off).to(DEV)
    out = torch.empty(T, E, dtype=BF, device=DEV)
    _hip.layernorm_f32(x32, w, b, 1e-5, out)
    ref, bound, pre = eb.layernorm_reference(x32, w, b, 1e-5, 'bf16')
    record('layernorm f32', eb.assert_bounded(out, ref, bound, f'layernorm_f32 {T}x{E} {kind}'))
    if out.numel() >= 10 ** 6:
        record_bias('layernorm f32', out, ref, pre, 'bf16')
    # split: fp32 in -> bf16 pair (+ fp32 copy), checked form with the overflow flag; and the bf16 / fp16 pair inputs
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    o32 = torch.empty(T, E, dtype=torch.float32, device=DEV)
    pr = _hip.layernorm_split(x32, w, b, 1e-5, E, out32=o32, overflow_flag=flag)
    _, pbound, ppre = eb.layernorm_reference(x32, w, b, 1e-5, 'bf16', pair=True)
    record('layernorm split', eb.assert_bounded(pr[:, :E].double() + pr[:, E:].double(), ref, pbound, 'layernorm_split pair'))
    record('layernorm split', eb.assert_bounded(o32, ref, ppre + eb.out_round(ref, ppre, 'fp32'), 'layernorm_split fp32'))
    assert int(flag.item()) == 0
    for dt in (BF, H16):
        hi = x32.to(dt)
        xp = torch.cat((hi, (x32 - hi.float()).to(dt)), 1).contiguous()
        xin = xp[:, :E].double() + xp[:, E:].double()
        refp, pb, _ = eb.layernorm_reference(xin, w, b, 1e-5, 'bf16', pair=True)
        pr = _hip.layernorm_split(xp, w, b, 1e-5, E)
        record('layernorm split', eb.assert_bounded(pr[:, :E].double() + pr[:, E:].double(), refp, pb, f'layernorm_split {dt} pair in'))


@pytest.mark.parametrize('d,H', [(16, 8), (32, 8), (64, 4), (128, 2)])
def test_rotary_forms(d, H):
    lengths = [1, 63, 64, 65, 700]
    T, E = sum(lengths), H * d
    cu = cu_of(lengths)
    pos, _ = _hip.seq_positions(cu, T)
    for dt in (BF, H16):
        qkv = rnd((T, 3 * E), d, 1.5, dtype=dt)
        cos, sin = (t.to(dt).to(DEV) for t in O.rotary_tables(max(lengths), d, torch.float32))
        g = qkv.clone()
        _hip.rotary_(g[:, :E], g[:, E:2 * E], cos, sin, pos, H)
        for blk in range(2):
            x = qkv[:, blk * E:(blk + 1) * E].double().view(T, H, d)
            r_, e_ = eb.rotary_bound(x, torch.zeros_like(x), cos, sin, pos)
            r_, e_ = r_.reshape(T, E), e_.reshape(T, E)
            got = g[:, blk * E:(blk + 1) * E]
            record(f'rotary {eb.fmt_of(dt)}', eb.assert_bounded(got, r_, e_ + eb.out_round(r_, e_, dt), f'rotary {dt} d{d} blk {blk}'))
            if got.numel() >= 2 * 10 ** 5:
                record_bias(f'rotary {eb.fmt_of(dt)}', got, r_, e_, dt)
        assert torch.equal(g[:, 2 * E:], qkv[:, 2 * E:])
    # split forms: pairs with fp32 tables, in place on 2H heads
    cos32, sin32 = (t.to(DEV) for t in O.rotary_tables(max(lengths), d, torch.float32))
    for dt in (BF, H16):
        x = (torch.randn(T, 2 * E, generator=torch.Generator().manual_seed(d)) * 1.5).to(DEV)
        hi = x.to(dt)
        p = torch.cat((hi, (x - hi.float()).to(dt)), 1).contiguous()
        xin = (p[:, :2 * E].double() + p[:, 2 * E:].double()).view(T, 2 * H, d)
        _hip.rotary_split_(p, 2 * E, cos32, sin32, pos, 2 * H, d)
        r_, e_ = eb.rotary_bound(xin, eb.U32 * xin.abs(), cos32, sin32, pos)       # hi + lo formed in fp32: one rounding
        r_, e_ = r_.reshape(T, 2 * E), e_.reshape(T, 2 * E)
        got = p[:, :2 * E].double() + p[:, 2 * E:].double()
        record('rotary split', eb.assert_bounded(got, r_, e_ + eb.out_round(r_, e_, dt, pair=True), f'rotary_split {dt} d{d}'))


def _qk_norm_call(form, q, k, wq, wk, bq, bk, cos, sin, pos, H, q_scale, sumsq):
    lib = _hip.load()
    T, E = q.shape
    d = E // H
    s = torch.cuda.current_stream().cuda_stream
    args = (q.data_ptr(), k.data_ptr(), q.stride(0), wq.data_ptr(), wk.data_ptr(), bq.data_ptr(), bk.data_ptr(), ctypes.c_float(1e-5),
            cos.data_ptr(), sin.data_ptr(), pos.data_ptr(), T, H, d, cos.shape[0])
    if form == 'bf16':
        rc = lib.esme_hip_qk_norm_rotary(*args, s)
    elif form == 'bf16_scaled':
        rc = lib.esme_hip_qk_norm_rotary_scaled(*args, ctypes.c_float(q_scale), s)
    elif form == 'f16':
        rc = lib.esme_hip_qk_norm_rotary_f16(*args, s)
    elif form == 'f16_guarded':
        rc = lib.esme_hip_qk_norm_rotary_f16_guarded(*args, sumsq.data_ptr(), s)
    else:
        rc = lib.esme_hip_qk_norm_rotary_f16_scaled(*args, ctypes.c_float(q_scale), sumsq.data_ptr(), s)
    assert rc == 0, lib.esme_hip_last_error()


@pytest.mark.parametrize('form', ['bf16', 'bf16_scaled', 'f16', 'f16_guarded', 'f16_scaled'])
@pytest.mark.parametrize('d,H', [(64, 15), (32, 8)])
def test_qk_norm_rotary_forms(form, d, H):
    """LayerNorm over H*d, then (bf16 forms) one bf16 rounding, rotary, q_scale, the output rounding (rowops.hip qk_norm_rotary_kernel)."""
    lengths = [100, 1, 37, 260, 700]
    T, E = sum(lengths), H * d
    cu = cu_of(lengths)
    pos, _ = _hip.seq_positions(cu, T)
    dt = H16 if form.startswith('f16') else BF
    qkv = rnd((T, 3 * E), d + len(form), 2.0, dtype=dt, offset=0.3)
    wq, bq = _ln_params(E, 1)
    wk, bk = _ln_params(E, 2)
    cos, sin = (t.to(dt).to(DEV) for t in O.rotary_tables(max(lengths), d, torch.float32))
    qs = 0.125 * LOG2E if form.endswith('scaled') else None
    sumsq = torch.zeros(2, H, dtype=torch.int32, device=DEV)
    g = qkv.clone()
    _qk_norm_call(form, g[:, :E], g[:, E:2 * E], wq, wk, bq, bk, cos, sin, pos, H, qs, sumsq)
    torch.cuda.synchronize()
    for blk, (w, b) in enumerate(((wq, bq), (wk, bk))):
        x = qkv[:, blk * E:(blk + 1) * E]
        y, _, pre = eb.layernorm_reference(x, w, b, 1e-5, 'bf16')
        if dt == BF:                                                    # the bf16 form rounds the LayerNorm output first
            pre = pre + eb.out_round(y, pre, 'bf16')
        r_, e_ = eb.rotary_bound(y.view(T, H, d), pre.view(T, H, d), cos, sin, pos, qs if blk == 0 else None)
        r_, e_ = r_.reshape(T, E), e_.reshape(T, E)
        record(f'qk_norm_rotary {form}', eb.assert_bounded(g[:, blk * E:(blk + 1) * E], r_, e_ + eb.out_round(r_, e_, dt),
                                                          f'qk_norm_rotary {form} d{d} blk {blk}'))
        if dt == H16 and d == 64:       # (the bf16 forms round the LayerNorm output first: half an ulp before the rotation, nothing qualifies)
            record_bias(f'qk_norm_rotary {form}', g[:, blk * E:(blk + 1) * E], r_, e_, dt)
    assert torch.equal(g[:, 2 * E:], qkv[:, 2 * E:])


@pytest.mark.parametrize('T,E', [(1, 64), (4099, 1280)])
def test_residual_f32_and_stream_operand(T, E):
    x32 = (torch.randn(T, E, generator=torch.Generator().manual_seed(T)) * 3).to(DEV)
    o = rnd((T, E), E, 2.0)
    for init in (False, True):
        xs = x32.clone()
        x16 = torch.empty(T, E, dtype=BF, device=DEV)
        sums = torch.empty(1, T, 2, dtype=torch.float32, device=DEV)
        _hip.residual_f32_(xs, o, 0.37, x16, sums, init=init)
        ref = (0.0 if init else x32.double()) + float(np.float32(0.37)) * o.double()
        record('residual_f32', eb.assert_bounded(xs, ref, eb.half_ulp(ref, 'fp32'),
                                                 f'residual_f32 init={init}'))      # alpha * o or fma: one rounding (rowops.hip:175, :179, residual_f32_kernel)
        assert torch.equal(x16, xs.to(BF))
        if xs.numel() >= BIAS_MIN_ELEMENTS:
            record_bias('residual_f32', xs, ref, torch.zeros_like(ref), 'fp32')
        v = xs.double()
        sb = torch.stack((eb.C_DOT * eb.U32 * math.sqrt(E) * v.norm(dim=1), eb.C_DOT * eb.U32 * math.sqrt(E) * (v * v).norm(dim=1)), 1)
        record('row sums', eb.assert_bounded(sums[0], torch.stack((v.sum(1), (v * v).sum(1)), 1), sb, 'residual_f32 sums'))
    # stream_operand: plain (bf16 / fp16 rounding, bit for bit), pair (scaled), guarded (col_absmax)
    for dt in (BF, H16):
        x16 = torch.empty(T, E, dtype=dt, device=DEV)
        sums = torch.empty(1, T, 2, dtype=torch.float32, device=DEV)
        _hip.stream_operand(x32, x16, sums)
        assert torch.equal(x16, x32.to(dt))
        v = x16.double()
        sb = torch.stack((eb.C_DOT * eb.U32 * math.sqrt(E) * v.norm(dim=1), eb.C_DOT * eb.U32 * math.sqrt(E) * (v * v).norm(dim=1)), 1)
        record('row sums', eb.assert_bounded(sums[0], torch.stack((v.sum(1), (v * v).sum(1)), 1), sb, f'stream_operand sums {dt}'))
        scale = (0.75 + 0.5 * torch.rand(E, generator=torch.Generator().manual_seed(1))).to(DEV)
        pair = torch.empty(T, 2 * E, dtype=dt, device=DEV)
        cmax = torch.zeros(E, dtype=torch.int32, device=DEV)
        _hip.stream_operand(x32, pair, sums, pair=True, scale=scale, col_absmax=cmax)
        ref = x32.double() * scale.double()
        pre = eb.U32 * ref.abs()                                          # scale * x32: one fp32 product
        got = pair[:, :E].double() + pair[:, E:].double()
        record('stream_operand pair', eb.assert_bounded(got, ref, pre + eb.out_round(ref, pre, dt, pair=True), f'stream_operand pair {dt}'))
        cm = cmax.view(torch.float32).double()
        assert bool(((cm - ref.abs().amax(0)).abs() <= eb.U32 * cm * 2).all()), 'col_absmax'


@pytest.mark.parametrize('dt', [BF, torch.float32])
def test_segment_mean_and_row_sums(dt):
    lengths = [1, 2, 63, 64, 65, 700, 1253, 0, 5]
    cu = cu_of(lengths)
    T, E = sum(lengths), 640
    x = rnd((T, E), 11, 2.0, dtype=dt, offset=0.5)
    got = _hip.segment_mean(x, cu)
    cl = cu.tolist()
    ref = torch.zeros(len(lengths), E, dtype=torch.float64, device=DEV)
    pre = torch.zeros_like(ref)
    for i, (s0, s1) in enumerate(zip(cl[:-1], cl[1:])):
        if s1 > s0:
            xs = x[s0:s1].double()
            ref[i] = xs.mean(0)
            pre[i] = eb.C_DOT * eb.U32 * math.sqrt(s1 - s0) * xs.norm(dim=0) / (s1 - s0) + 2 * eb.U32 * ref[i].abs()
    record('segment_mean', eb.assert_bounded(got, ref, pre + eb.out_round(ref, pre, dt), f'segment_mean {dt}'))
    if dt == BF:
        s = _hip.row_sums(x)[0]
        v = x.double()
        sb = torch.stack((eb.C_DOT * eb.U32 * math.sqrt(E) * v.norm(dim=1), eb.C_DOT * eb.U32 * math.sqrt(E) * (v * v).norm(dim=1)), 1)
        record('row sums', eb.assert_bounded(s, torch.stack((v.sum(1), (v * v).sum(1)), 1), sb, 'row_sums'))


@pytest.mark.parametrize('V', [33, 64])
@pytest.mark.parametrize('dt', [BF, torch.float32])
def test_softmax_rows(V, dt):
    T = 5000
    buf = rnd((T, 80), V, 4.0, dtype=dt)
    x = buf[:, 4:4 + V] if dt == torch.float32 else buf[:, 8:8 + V]      # strided rows (16-byte aligned starts)
    for log in (True, False):
        got = _hip.softmax_rows(x, log)
        ref, bound, pre = eb.softmax_reference(x, log, dt)
        record(f'softmax_rows {eb.fmt_of(dt)}', eb.assert_bounded(got, ref, bound, f'softmax_rows V={V} {dt} log={log}'))
        if dt == BF:
            record_bias(f'softmax_rows bf16 log={log}', got, ref, pre, 'bf16')


def test_pair_to_f32_bit_equal():
    T, E = 777, 640
    for dt in (BF, H16):
        x = (torch.randn(T, E, generator=torch.Generator().manual_seed(2)) * 5).to(DEV)
        hi = x.to(dt)
        p = torch.cat((hi, (x - hi.float()).to(dt)), 1).contiguous()
        assert torch.equal(_hip.pair_to_f32(p), hi.float() + p[:, E:].float())
        wide = torch.cat((hi, torch.zeros(T, 64, dtype=dt, device=DEV), p[:, E:]), 1).contiguous()   # [hi | ext | lo]
        assert torch.equal(_hip.pair_to_f32(wide, E), hi.float() + p[:, E:].float())


def test_embed_positions_bit_equal():
    V, E, P, T = 33, 320, 1030, 2000
    table = rnd((V, E), 1)
    pos_table = rnd((P, E), 2, 0.5)
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(0, V, (T,), generator=g).to(DEV)
    tok[::7] = 32
    lengths = [1, 999, 1000]
    pos, _ = _hip.seq_positions(cu_of(lengths), T)
    tr = table[tok].float()
    tr[tok == 32] = 0.0
    s = tr + pos_table[(pos.long() + 2).clamp(max=P - 1)].float()
    assert torch.equal(_hip.embed_positions(tok, table, pos_table, pos, 2, mask_idx=32, f32=True), s)
    assert torch.equal(_hip.embed_positions(tok, table, pos_table, pos, 2, mask_idx=32), s.to(BF))
