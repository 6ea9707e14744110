"""The cases that hold the persistent 256 x 256 GEMM kernels (all 17 PERSIST = true instantiations) to the float64 bound, and the
checks every case runs.  Imports without a GPU: tests/test_gemm_path_cpu.py pushes the case table through the launcher to prove that
it reaches every persistent instantiation, tests/test_gemm_persistent_cpu.py runs the checks on an emulation with seam defects, and
tests/test_gemm_persistent_bounds_gpu.py runs them on the kernels.

A persistent workgroup walks several tiles: it fetches the next tile's first K-tile and LayerNorm strip under the current tile's
two-pass epilogue and carries the stage-buffer parity over the seam.  What can go wrong there shows in a tile at walk position >= 1
(tests/gemm_path.py: walks), so the shapes are the smallest with walks of different lengths, and the K are 1, 2, 3 and 5 K-tiles of
64 (odd counts flip the parity from tile to tile, even counts keep it; with one K-tile the prefetched tile is the whole product).
"""
import torch

import error_bounds as eb
import gemm_operands as ops
import gemm_path as gp
from gemm_operands import BF, H16

EPI_NONE, EPI_GELU, EPI_RESIDUAL, EPI_SWIGLU = 0, 1, 2, 3
FORMS = gp.PERSISTENT_FORMS                                  # the 17 forms with a persistent twin
BASE_K = (64, 128, 192, 320)
# the further shapes and the rasters run these four: plain with bias, GELU with LayerNorm fold, statistics on the fp32 stream in bf16 and fp16
SEAM_FORMS = ('bf16_none', 'bf16_gelu_ln', 'bf16_r32_stats', 'f16_r32_stats')
SEAM_K = (64, 192)
SEAM_SHAPES = ('two_walks', 'r7', 'three_walks')
RASTERS = [(0, 0), (1, 1), (3, 4), (5, 7), (64, 1), (2, 64)]        # those of test_error_bounds_gpu.py::test_gemm_options_bit_equal
RASTER_K = 192
# forms whose last step is one rounding of a value whose pre-rounding bound stays far under 0.05 ulp of the output format at these shapes:
# they take the rounding-bias check (the fp32-stream forms through C, the 16-bit rounding of the stream).  Not the GELU forms after a
# LayerNorm fold (the degree-5 polynomial alone is 0.19 of half an ulp) and not fp16 GELU (the polynomial's error is stated in bf16 ulps).
BIAS_FORMS = ('bf16_none', 'bf16_gelu', 'bf16_swiglu', 'bf16_resid', 'bf16_resid_stats', 'bf16_none_ln', 'bf16_swiglu_ln',
              'bf16_r32', 'bf16_r32_stats', 'f16_none', 'f16_none_ln', 'f16_r32', 'f16_r32_stats')


def flags(form):
    epi, _, lnf, stats, r32, _, f16, _ = gp.FORMS[form]
    return epi, bool(lnf), bool(stats), bool(r32), bool(f16)


def shape(kind, form, ncu):
    """(M, N) of a case on a device with `ncu` (a multiple of 8) persistent workgroups.
      base         N = 520 (three tile columns, the last 8 wide; 576 where the form needs N % 64 == 0), ceil((2 ncu + 1) / 3) row tiles,
                   the last one row deep: the smallest launch with walks of different lengths
      two_walks    exactly 2 ncu tiles in one ragged tile column (N = 192): every walk has length 2; two_walks_less: 2 ncu - 1, per tile
      r7           2 ncu + 7 tiles: the XCD ranges have unequal length
      three_walks  at least 3 ncu + 1 tiles in three columns: every workgroup walks three tiles or more"""
    epi, _, stats, _, _ = flags(form)
    wide = 576 if stats or epi == EPI_SWIGLU else 520
    n, tm = {'base': (wide, -(-(2 * ncu + 1) // 3)), 'two_walks': (192, 2 * ncu), 'two_walks_less': (192, 2 * ncu - 1),
             'r7': (192, 2 * ncu + 7), 'three_walks': (wide, -(-(3 * ncu + 1) // 3))}[kind]
    return (tm - 1) * 256 + 1, n


def case_table():
    """Every (form, shape kind, K, raster) the GPU file runs with persist = 1."""
    rows = [(f, 'base', k, (0, 0)) for f in FORMS for k in BASE_K]
    rows += [(f, s, k, (0, 0)) for f in SEAM_FORMS for s in SEAM_SHAPES for k in SEAM_K]
    rows += [(f, 'base', RASTER_K, r) for f in SEAM_FORMS for r in RASTERS[1:]]
    return rows


def walk_lengths(M, N, ncu):
    tm, tn = gp.tile_counts(M, N)
    owner, _ = gp.walks(tm * tn, ncu)
    return [owner.count(b) for b in range(ncu & ~7)]


def assert_premise(form, kind, M, N, ncu):
    """What a case is there for: persist = 1 runs the persistent kernel, persist = 0 does not, and the walks have the lengths the shape is meant to give."""
    assert gp.runs_persistent(form, M, N, 2, 1, True, ncu), f'{form} {M}x{N}: persist=1 does not reach the persistent kernel on {ncu} compute units'
    assert not gp.runs_persistent(form, M, N, 2, 0, True, ncu)
    lens = walk_lengths(M, N, ncu)
    if kind == 'two_walks':
        assert set(lens) == {2}, sorted(set(lens))
    elif kind == 'three_walks':
        assert min(lens) >= 3, min(lens)
    else:
        assert max(lens) >= 3 and min(lens) == 2, (min(lens), max(lens))     # walk positions 0, 1 and 2 are present, and not in every walk
    if kind == 'r7':
        assert (gp.tile_counts(M, N)[0] * gp.tile_counts(M, N)[1]) & 7 == 7


# ------------------------------------------------------------------ operands

def operands(form, M, N, K, dev=ops.DEV, hip=None):
    """The operands of one call of `form`, by the recipes of tests/test_error_bounds_gpu.py (gemm_operands.py).  `hip` (esme._hip): row sums and
    the fp16 stream come from the library's own kernels; None (CPU emulation, bf16 forms only): fp32 row sums formed here."""
    epi, lnf, stats, r32, f16 = flags(form)
    o = dict(form=form, M=M, N=N, K=K, epi=epi, lnf=lnf, stats=stats, r32=r32, f16=f16, fmt='fp16' if f16 else 'bf16',
             alpha=1.0, bias=None, resid=None, x32=None, ln=None, dim=K)
    if lnf and not f16:
        x, wp, c1, c2 = ops.ln_fold_operands(M, K, N, 5 + K, 'dc20', dev)
        xf = x.float()
        sums = hip.row_sums(x) if hip is not None else torch.stack((xf.sum(1), (xf * xf).sum(1)), 1)[None].contiguous()
        o.update(a=x, w=wp, w_nat=wp, c1_nat=c1, c2_nat=c2, sums=sums)
    elif lnf:
        # the fp32 stream with three massive channels; past one K-tile the operand is [hi | extension tile] of the fp16 pair stream over K = E + 64
        E = K - 64 if K > 64 else K
        sel = torch.tensor([5, E // 2, E - 3], dtype=torch.int32)
        x32, wp, wext, c1, c2 = (t.to(dev) for t in ops.f16_ln_fold_operands(M, E, N, 90 + K, sel))
        sums = torch.empty(1, M, 2, dtype=torch.float32, device=dev)
        if K > 64:
            pair = torch.zeros(M, 2 * E + 64, dtype=H16, device=dev)
            hip.stream_operand(x32, pair, sums, pair=True, ext_sel=sel.to(dev))
            a, wp = pair[:, :E + 64], wext
        else:
            a = torch.empty(M, E, dtype=H16, device=dev)
            hip.stream_operand(x32, a, sums)
        o.update(a=a, w=wp, w_nat=wp, c1_nat=c1, c2_nat=c2, sums=sums, dim=E)
    elif epi == EPI_RESIDUAL:
        a, w, b, r, x32 = ops.residual_stream_operands(M, N, K, dev)
        if f16:
            a, w, b = ops.f16_operands(M, N, K, dev)
        o.update(a=a, w=w, bias=b, alpha=0.5, resid=None if r32 else r, x32=x32 if r32 else None)
    elif f16:
        a, w, b = ops.f16_operands(M, N, K, dev)
        o.update(a=a, w=w, bias=b)
    else:
        a, w, b, _ = ops.plain_operands(M, N, K, dev)
        o.update(a=a, w=w, bias=None if epi == EPI_SWIGLU else b)
    c1, c2 = o.get('c1_nat'), o.get('c2_nat')
    if epi == EPI_SWIGLU:                                      # gate = the first N / 2 rows, fc the rest; the kernel reads them interleaved
        F = N // 2
        o['w_nat'] = o['w']
        o['w'] = ops.swiglu_pack(o['w'][:F], o['w'][F:])
        if lnf:
            c1, c2 = (ops.swiglu_pack(c[:F], c[F:]) for c in (o['c1_nat'], o['c2_nat']))
    if lnf:
        o['ln'] = (o['sums'], o['dim'], 1e-5, c1, c2)
    return o


def nan_outputs(o, nblk, dev):
    """C, stats_out and (a copy of) the fp32 stream as a call receives them.  C and stats_out hold NaN, so that a tile that is never written
    fails the finiteness check; the fp32 stream is read and written in place, so an unwritten tile keeps the old stream and misses the bound."""
    n_out = o['N'] // 2 if o['epi'] == EPI_SWIGLU else o['N']
    out = {'C': torch.full((o['M'], n_out), float('nan'), dtype=H16 if o['f16'] else BF, device=dev)}
    if o['stats']:
        out['stats'] = torch.full((nblk, o['M'], 2), float('nan'), dtype=torch.float32, device=dev)
    if o['r32']:
        out['x32'] = o['x32'].clone()
    return out


def launch(o, hip, persist, raster=(0, 0)):
    """One call under gemm_options(tile=2, persist=persist, raster=raster) on NaN-filled outputs."""
    with hip.gemm_options(tile=2, persist=persist, raster=raster):
        out = nan_outputs(o, hip.stats_blocks(o['M'], o['N']), o['a'].device)
        hip.gemm_fused(o['a'], o['w'], o['bias'], o['epi'], o['resid'], o['alpha'], out=out['C'], ln=o['ln'], stats_out=out.get('stats'),
                       resid32=out.get('x32'))
    return out


# ------------------------------------------------------------------ references

def references(o, got):
    """[(output name, got, ref, bound, pre or None)] of one call: the recipes of tests/test_error_bounds_gpu.py, unchanged."""
    fmt, epi = o['fmt'], o['epi']
    checks = []
    if '_static' not in o:                                     # the float64 product is formed once per case and shared by both results
        o['_static'] = _static_references(o)
    for name, ref, bound, pre in o['_static']:
        checks.append((name, got[name], ref, bound, pre))
    if o['r32']:
        assert torch.equal(got['C'], got['x32'].to(got['C'].dtype)), f'{o["form"]}: C is not the rounding of the updated stream'
    if o['stats']:
        s_ref, sb = ops.stats_reference(got['C'], got['stats'].shape[0])
        checks.append(('stats', got['stats'].double().sum(0), s_ref, sb, None))
    return checks


def _static_references(o):
    fmt, epi = o['fmt'], o['epi']
    checks = []
    if o['lnf']:
        y, pre = eb.ln_fold_reference(o['a'], o['w_nat'], o['c1_nat'], o['c2_nat'], 1e-5, o['sums'], dim=o['dim'])
        if epi == EPI_NONE:
            checks.append(('C', y, pre + eb.out_round(y, pre, fmt), pre))
        elif epi == EPI_GELU:
            gpre, gv = eb.gelu_bound(y, pre, 5), eb.gelu64(y)          # the LN-folded site runs the degree-5 polynomial
            checks.append(('C', gv, gpre + eb.out_round(gv, gpre, fmt), gpre))
        else:
            F = o['N'] // 2
            checks.append(('C', *eb.swiglu_bound(y[:, :F], y[:, F:], pre[:, :F], pre[:, F:], fmt)))
    elif epi == EPI_SWIGLU:
        F = o['N'] // 2
        checks.append(('C', *eb.swiglu_reference(o['a'], o['w_nat'][:F], o['w_nat'][F:], fmt)))
    elif o['r32']:
        # x32 <- fma(alpha, acc + bias, x32), one rounding; C = its 16-bit rounding, bit for bit
        y, _, pre = eb.gemm_reference(o['a'], o['w'], o['bias'])
        ref32 = o['x32'].double() + o['alpha'] * y
        pre32 = o['alpha'] * pre + eb.U32 * ref32.abs()
        checks.append(('x32', ref32, pre32, None))
        checks.append(('C', ref32, pre32 + eb.out_round(ref32, pre32, fmt), pre32))
    else:
        name = {EPI_NONE: 'none', EPI_GELU: 'gelu', EPI_RESIDUAL: 'residual'}[epi]
        checks.append(('C', *eb.gemm_reference(o['a'], o['w'], o['bias'], name, resid=o['resid'], alpha=o['alpha'], out_fmt=fmt)))
    return checks


# ------------------------------------------------------------------ the checks

def seam_layout(positions, bn_out):
    """gemm_layout(256, bn_out) with the tile's walk position beside it (bn_out: output columns per tile; 128 under SwiGLU)."""
    base = eb.gemm_layout(256, bn_out)

    def where(idx, shp):
        return base(idx, shp) + f', walk position {positions[idx[0] // 256][idx[1] // bn_out]}'
    return where


def per_position(got, ref, bound, positions, bn_out):
    """Worst err / bound of an (M, n_out) output per walk position: [position 0, position 1, positions >= 2] (a non-finite element counts as inf)."""
    ratio = (got.double() - ref.to(got.device).double()).abs() / bound.to(got.device).double()
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float('inf')))
    M, n = ratio.shape
    tm, tn = len(positions), len(positions[0])
    full = torch.zeros(tm * 256, tn * bn_out, dtype=ratio.dtype, device=ratio.device)
    full[:M, :n] = ratio
    per_tile = full.view(tm, 256, tn, bn_out).amax((1, 3))
    pos = torch.tensor(positions, device=ratio.device).clamp(max=2)
    return [float(per_tile[pos == p].max()) if bool((pos == p).any()) else 0.0 for p in range(3)]


def check_written(what, got):
    """(b) C and stats_out were handed over full of NaN: a tile that was never written leaves some."""
    for name in ('C', 'stats'):
        if name in got:
            bad = ~torch.isfinite(got[name].float())
            assert not bool(bad.any()), f'{what} {name}: {int(bad.sum())} non-finite elements (first at {tuple(int(i) for i in bad.nonzero()[0])}): a tile was not written'


def check_bounded(what, o, got, ncu, raster=(0, 0), ledger=None, tag='persistent'):
    """(c) and (e): every output inside its float64 bound, a failure located by tile and walk position; the rounding bias of the forms in
    BIAS_FORMS.  Returns {output: [worst err / bound at walk position 0, 1, >= 2]}."""
    positions = gp.walk_positions(o['M'], o['N'], o['K'], ncu, *raster)
    bn_out = 128 if o['epi'] == EPI_SWIGLU else 256
    where = seam_layout(positions, bn_out)
    table = {}
    for name, g, ref, bound, pre in references(o, got):
        if name != 'stats':
            table[name] = per_position(g, ref, bound, positions, bn_out)
        try:
            worst = eb.assert_bounded(g, ref, bound, f'{what} {tag} {name}', where if name != 'stats' else None)
        except AssertionError as e:
            row = table.get(name)
            raise AssertionError(f'{e}' + (f'; worst err / bound at walk position 0 / 1 / >= 2: {row[0]:.3g} / {row[1]:.3g} / {row[2]:.3g}' if row else '')) from None
        if ledger is not None:
            ledger.record(f'{o["form"]} {tag} {name}', worst)
            if name == 'C' and o['form'] in BIAS_FORMS and g.numel() >= ops.BIAS_MIN_ELEMENTS:
                ledger.record_bias(f'{o["form"]} {tag}', g, ref, pre, o['fmt'])
    return table


def check_same_bits(what, got_p, got_t):
    """(d) the persistent kernel writes the bits of the per-tile kernel: C, the statistics rows and the fp32 stream."""
    for name in got_p:
        assert torch.equal(got_p[name], got_t[name]), f'{what}: {name} of the persistent kernel differs from the per-tile kernel'


def hold(what, o, got_p, got_t, ncu, raster=(0, 0), ledger=None):
    """Checks (b) to (e) of one case on the persistent outputs `got_p` and the per-tile outputs `got_t` (dicts of C / stats / x32).
    Returns the per-walk-position tables of both results (the per-tile result's rows are the comparison: same tiles, no seam)."""
    tables = {}
    for tag, got in (('persistent', got_p), ('per tile', got_t)):
        check_written(f'{what} {tag}', got)
        tables[tag] = check_bounded(what, o, got, ncu, raster, ledger, tag)
    check_same_bits(what, got_p, got_t)
    return tables
