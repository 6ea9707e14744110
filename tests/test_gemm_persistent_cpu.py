"""The checks that hold the persistent GEMM kernels (tests/gemm_persistent_cases.py) see a seam defect, shown on the CPU.

`emulate` is a float32 / bf16 restatement of a tiled 256 x 256 GEMM whose tiles are produced in the order of the persistent kernel's walks
(tests/gemm_path.py: walks), with the state a workgroup carries over the tile seam made explicit: the prefetched first K-tile, the
LayerNorm strip, the stage-buffer parity, the column-block index of the statistics rows, the origin of the second store pass.  Each
entry of DEFECTS breaks one of them the way a change to the seam could; the clean emulation passes the checks the GPU file runs, and
every defect is rejected by the check named beside it.  The shape is the base shape of the GPU file at the smallest device on which
the launcher takes the persistent kernel at all, 8 compute units: 18 tiles in three columns, walks of length 3 and 2.  (On fewer than
8 compute units `ncu & ~7` is 0: there is no persistent launch, and no split to restate.)
"""
import math

import pytest
import torch

import gemm_path as gp
import gemm_persistent_cases as pc
from gemm_operands import BF

NCU = 8
FORMS = ('bf16_none', 'bf16_gelu_ln', 'bf16_r32_stats')
DEFECTS = {
    # name: (forms it applies to, the checks that must reject it)
    'stale_first_ktile': (FORMS, 'c'),                     # K-tile 0 of a tile at position >= 1 is the previous tile's (the prefetch never landed)
    'stale_ln_strip': (('bf16_gelu_ln',), 'c'),            # row statistics / c1 / c2 of the previous tile applied at position >= 1
    'parity_not_flipped': (FORMS, 'c'),                    # odd K-tile counts: the last K-tile of position >= 1 is read from the other stage buffer
    'range_end_short': (FORMS, 'b'),                       # pid_end one short: the last id of every XCD range is never walked
    'stats_prev_block': (('bf16_r32_stats',), 'dcb'),      # statistics rows written under the previous tile's column-block index (its own block keeps the NaN)
    'second_pass_next_origin': (FORMS, 'cb'),              # m0 moved before em0 was latched: the second pass lands at the next tile's origin
}


def _epilogue(o, acc, rows, cols, strip):
    """fp32 epilogue of one 256 x 256 tile (padded rows / columns included): rows, cols index the padded operands; `strip` = (rows, cols) the
    LayerNorm strip was fetched for."""
    v = acc
    if o['lnf']:
        srows, scols = strip
        s = o['_sums'][srows]
        inv = torch.tensor(1.0 / o['dim'], dtype=torch.float32)
        mean = s[:, 0] * inv
        var = s[:, 1] * inv - mean * mean
        rstd = torch.rsqrt(var + torch.tensor(1e-5, dtype=torch.float32))
        c1, c2 = o['_c1'][scols], o['_c2'][scols]
        v = rstd[:, None] * acc + ((-(rstd * mean))[:, None] * c1[None, :] + c2[None, :])
    elif o['bias'] is not None:
        v = acc + o['_bias'][cols][None, :]
    if o['epi'] == pc.EPI_GELU:
        v = 0.5 * v * (1.0 + torch.erf(v * (1.0 / math.sqrt(2.0))))
    return v


def emulate(o, ncu=NCU, persistent=True, defect=None):
    """C / stats / x32 of one call as nan_outputs hands them over, written tile by tile: in the persistent kernel's walks, or one tile per workgroup."""
    assert defect is None or defect in DEFECTS, defect
    M, N, K = o['M'], o['N'], o['K']
    tm, tn, gm, gn = gp.raster(M, N, K)
    tiles, nkt = tm * tn, K // 64
    out = pc.nan_outputs(o, tn, 'cpu')
    pad = lambda t, n: torch.cat((t.float(), torch.zeros(n - t.shape[0], *t.shape[1:])), 0)
    A, W = pad(o['a'], tm * 256), pad(o['w'], tn * 256)
    if o['lnf']:
        o['_sums'], o['_c1'], o['_c2'] = pad(o['sums'].sum(0), tm * 256), pad(o['ln'][3], tn * 256), pad(o['ln'][4], tn * 256)
    if o['bias'] is not None:
        o['_bias'] = pad(o['bias'], tn * 256)
    if persistent:
        owner, position = gp.walks(tiles, ncu)
        todo = [sorted((p for p in range(tiles) if owner[p] == b), key=lambda p: position[p]) for b in range(ncu & ~7)]
        if defect == 'range_end_short':
            q, r = tiles >> 3, tiles & 7
            ends = {(x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + q + (1 if x < r else 0) - 1 for x in range(8)}
            todo = [[p for p in walk if p not in ends] for walk in todo]
    else:
        todo = [[p] for p in range(tiles)]
    span = lambda t: torch.arange(t * 256, t * 256 + 256)
    ktile = lambda rows, cols, kt: A[rows, kt * 64:kt * 64 + 64] @ W[cols, kt * 64:kt * 64 + 64].T
    for walk in todo:
        prev = None                                           # (rows, cols, column tile) of the tile before this one in the walk
        for step, pid in enumerate(walk):
            i, j = gp.tile_coords(pid, tm, tn, gm, gn)
            rows, cols = span(i), span(j)
            acc = torch.zeros(256, 256)
            for kt in range(nkt):
                src = (rows, cols, kt)
                if prev is not None and kt == 0 and defect == 'stale_first_ktile':
                    src = (prev[0], prev[1], 0)
                if prev is not None and kt == nkt - 1 and nkt % 2 == 1 and defect == 'parity_not_flipped':
                    src = (rows, cols, kt - 1) if nkt > 1 else (prev[0], prev[1], 0)      # what the other buffer holds
                acc = acc + ktile(*src)
            strip = (prev[0], prev[1]) if prev is not None and defect == 'stale_ln_strip' else (rows, cols)
            v = _epilogue(o, acc, rows, cols, strip)
            if o['r32']:
                x = torch.zeros(256, 256)
                r1, c1 = min(M, i * 256 + 256), min(N, j * 256 + 256)
                x[:r1 - i * 256, :c1 - j * 256] = out['x32'][i * 256:r1, j * 256:c1]
                v = o['alpha'] * v + x                        # (alpha = 0.5: the product is exact, one rounding as in the kernel's fma)
            c16 = v.to(BF)
            # two store passes of 64-row slabs per 128-row wave tile
            for half in (0, 1):
                dst_i, dst_j = i, j
                if half == 1 and defect == 'second_pass_next_origin' and step + 1 < len(walk):
                    dst_i, dst_j = gp.tile_coords(walk[step + 1], tm, tn, gm, gn)
                for rr in ((torch.arange(256) % 128) // 64 == half).nonzero()[:, 0].tolist():
                    gr = dst_i * 256 + rr
                    if gr >= M:
                        continue
                    c1 = min(N, dst_j * 256 + 256) - dst_j * 256
                    out['C'][gr, dst_j * 256:dst_j * 256 + c1] = c16[rr, :c1]
                    if o['r32']:
                        out['x32'][gr, dst_j * 256:dst_j * 256 + c1] = v[rr, :c1]
            if o['stats']:
                blk = prev[2] if prev is not None and defect == 'stats_prev_block' else j
                cf = c16.float()[:, :min(N, j * 256 + 256) - j * 256]
                r1 = min(M, i * 256 + 256)
                out['stats'][blk, i * 256:r1, 0] = cf.sum(1)[:r1 - i * 256]
                out['stats'][blk, i * 256:r1, 1] = (cf * cf).sum(1)[:r1 - i * 256]
            prev = (rows, cols, j)
    return out


_CACHE = {}


def _case(form, K):
    """(operands, per-tile emulation) of one case, built once."""
    if (form, K) not in _CACHE:
        M, N = pc.shape('base', form, NCU)
        pc.assert_premise(form, 'base', M, N, NCU)
        o = pc.operands(form, M, N, K, dev='cpu')
        _CACHE[(form, K)] = o, emulate(o, persistent=False)
        pc.references(o, _CACHE[(form, K)][1])               # (forms the float64 reference once: o['_static'])
    return _CACHE[(form, K)]


def _written_only(o, got):
    """`got` with its never-written elements set to values inside the bound, so that (c) judges what WAS written, apart from (b)."""
    g = {k: v.clone() for k, v in got.items()}
    ref = {name: r for name, r, _, _ in o['_static']}
    fill = g['x32'] if 'x32' in g else ref['C']             # (fp32 stream: C stays the rounding of the stream, which kept its old value there)
    g['C'] = torch.where(torch.isfinite(g['C'].float()), g['C'], fill.to(g['C'].dtype))
    if 'stats' in g:
        g['stats'] = torch.where(torch.isfinite(g['stats']), g['stats'], torch.zeros_like(g['stats']))
    return g


@pytest.mark.parametrize('K', [64, 192])
@pytest.mark.parametrize('form', FORMS)
def test_clean_emulation_passes_the_checks(form, K):
    o, per_tile = _case(form, K)
    tables = pc.hold(f'emulated {form} K={K}', o, emulate(o), per_tile, NCU)
    for tag in tables:
        for name, row in tables[tag].items():
            assert max(row) <= 1.0 and row[1] > 0.0 and row[2] > 0.0, (tag, name, row)       # walk positions 1 and >= 2 hold tiles
    assert tables['persistent'] == tables['per tile']


@pytest.mark.parametrize('K', [64, 192])
@pytest.mark.parametrize('defect,form', [(d, f) for d, (forms, _) in DEFECTS.items() for f in forms])
def test_seam_defect_is_rejected_by_the_named_check(defect, form, K):
    o, per_tile = _case(form, K)
    got = emulate(o, defect=defect)
    what = f'emulated {form} K={K} {defect}'
    checks = DEFECTS[defect][1]
    if 'b' in checks:
        with pytest.raises(AssertionError, match='a tile was not written'):
            pc.check_written(what, got)
    else:
        pc.check_written(what, got)
    if 'c' in checks:
        with pytest.raises(AssertionError, match='out of bound') as e:
            pc.check_bounded(what, o, _written_only(o, got), NCU)
        if defect == 'stats_prev_block':
            assert ' stats:' in str(e.value)
        else:                                                   # the message names the walk position beside the tile
            assert 'walk position' in str(e.value), str(e.value)
            if defect in ('stale_first_ktile', 'stale_ln_strip', 'parity_not_flipped'):      # ... and these sit past the seam
                assert 'walk position 0:' not in str(e.value), str(e.value)
    if 'd' in checks or 'c' in checks:
        with pytest.raises(AssertionError, match='differs from the per-tile kernel'):
            pc.check_same_bits(what, got, per_tile)
    if defect == 'stale_first_ktile':                           # (e) the per-position table: position 0 as good as ever, a jump from position 1 on
        ref = {name: (r, b) for name, r, b, _ in o['_static']}
        clean = pc.per_position(per_tile['C'], *ref['C'], gp.walk_positions(o['M'], o['N'], K, NCU), 256)
        row = pc.per_position(got['C'], *ref['C'], gp.walk_positions(o['M'], o['N'], K, NCU), 256)
        assert row[0] == clean[0] <= 1.0 and row[1] > 10.0 and row[2] > 10.0, (row, clean)


@pytest.mark.parametrize('form', FORMS)
def test_parity_defect_is_invisible_at_an_even_k_tile_count(form):
    """Why both parities are in the GPU file's table: with 2 K-tiles lastbuf is the same for every tile of a walk, and the defect changes nothing."""
    o, per_tile = _case(form, 128)
    pc.hold(f'emulated {form} K=128 parity_not_flipped', o, emulate(o, defect='parity_not_flipped'), per_tile, NCU)


def test_walks_partition_the_tiles():
    """Every tile id belongs to exactly one workgroup, at consecutive walk positions, for the tile counts around two walks."""
    for ncu, counts in ((256, range(512, 531)), (8, range(8, 41)), (300, range(592, 600))):
        for tiles in counts:
            owner, position = gp.walks(tiles, ncu)           # (walks itself asserts that no id is taken twice)
            assert None not in owner and len(owner) == tiles
            for b in set(owner):
                ids = [p for p in range(tiles) if owner[p] == b]
                assert [position[p] for p in ids] == list(range(len(ids))), (ncu, tiles, b)
                assert all(y - x == (ncu & ~7) >> 3 for x, y in zip(ids, ids[1:]))
                assert b < (ncu & ~7)
    with pytest.raises(ValueError):
        gp.walks(9, 4)                                       # 4 compute units: ncu & ~7 = 0, the launcher never takes the persistent kernel
    assert not any(gp.runs_persistent('bf16_none', 256 * t, 256, 2, 1, True, 4) for t in (1, 9, 40, 4000))


def test_tile_coords_cover_the_grid():
    """The (gm, gn) raster maps the ids onto every (row tile, column tile) once, for groups that do not divide the grid."""
    for tm, tn in ((6, 3), (171, 3), (9, 10), (1, 1)):
        for gm, gn in pc.RASTERS:
            _, _, g_m, g_n = gp.raster(tm * 256, tn * 256, 64, gm, gn)
            seen = {gp.tile_coords(p, tm, tn, g_m, g_n) for p in range(tm * tn)}
            assert seen == {(i, j) for i in range(tm) for j in range(tn)}, (tm, tn, gm, gn)
