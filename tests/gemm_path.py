"""Which kernel a forward GEMM call runs, and how the persistent kernel walks its tiles: a pure-Python restatement of the launcher's
decision (csrc/gemm.hip: pick_tile, has_persistent_twin, launch_one, set_raster) and of the persistent kernel's split of the tile ids.

A GEMM test that means to exercise the persistent 256 x 256 kernel asserts its premise through `runs_persistent`: passing persist=1
does not force that kernel below 2 * (compute units & ~7) tiles.  tests/test_gemm_path_cpu.py pins every function here against the
launcher itself (tools/kernel_launch_log.cpp, host only), at 256, 4 and 300 compute units.  No torch, no GPU.
"""
import os
import re

# the shipped forms by the names of tools/kernel_launch_log.cpp: (epilogue, rotary head dim, LN fold, row statistics, fp32 stream, pair output,
# fp16 operands, fp16 pair stream) -- the kernel's template arguments but the tile and PERSIST.  Epilogues: 0 none, 1 GELU, 2 residual, 3 SwiGLU.
FORMS = {
    'bf16_none': (0, 0, 0, 0, 0, 0, 0, 0), 'bf16_none_ln': (0, 0, 1, 0, 0, 0, 0, 0),
    'bf16_rot16': (0, 16, 0, 0, 0, 0, 0, 0), 'bf16_rot32': (0, 32, 0, 0, 0, 0, 0, 0), 'bf16_rot64': (0, 64, 0, 0, 0, 0, 0, 0),
    'bf16_rot16_ln': (0, 16, 1, 0, 0, 0, 0, 0), 'bf16_rot32_ln': (0, 32, 1, 0, 0, 0, 0, 0), 'bf16_rot64_ln': (0, 64, 1, 0, 0, 0, 0, 0),
    'bf16_gelu': (1, 0, 0, 0, 0, 0, 0, 0), 'bf16_gelu_ln': (1, 0, 1, 0, 0, 0, 0, 0),
    'bf16_swiglu': (3, 0, 0, 0, 0, 0, 0, 0), 'bf16_swiglu_ln': (3, 0, 1, 0, 0, 0, 0, 0),
    'bf16_resid': (2, 0, 0, 0, 0, 0, 0, 0), 'bf16_resid_stats': (2, 0, 0, 1, 0, 0, 0, 0),
    'bf16_r32': (2, 0, 0, 0, 1, 0, 0, 0), 'bf16_r32_stats': (2, 0, 0, 1, 1, 0, 0, 0),
    'pair_none': (0, 0, 0, 0, 0, 1, 0, 0), 'pair_rot16': (0, 16, 0, 0, 0, 1, 0, 0), 'pair_rot32': (0, 32, 0, 0, 0, 1, 0, 0),
    'pair_rot64': (0, 64, 0, 0, 0, 1, 0, 0), 'pair_gelu': (1, 0, 0, 0, 0, 1, 0, 0), 'pair_swiglu': (3, 0, 0, 0, 0, 1, 0, 0),
    'f16pair_none': (0, 0, 1, 0, 0, 1, 1, 0), 'f16pair_rot16': (0, 16, 1, 0, 0, 1, 1, 0), 'f16pair_rot32': (0, 32, 1, 0, 0, 1, 1, 0),
    'f16pair_rot64': (0, 64, 1, 0, 0, 1, 1, 0),
    'f16_none': (0, 0, 0, 0, 0, 0, 1, 0), 'f16_none_ln': (0, 0, 1, 0, 0, 0, 1, 0),
    'f16_rot16_ln': (0, 16, 1, 0, 0, 0, 1, 0), 'f16_rot32_ln': (0, 32, 1, 0, 0, 0, 1, 0), 'f16_rot64_ln': (0, 64, 1, 0, 0, 0, 1, 0),
    'f16_gelu': (1, 0, 0, 0, 0, 0, 1, 0), 'f16_gelu_ln': (1, 0, 1, 0, 0, 0, 1, 0), 'f16_swiglu_ln': (3, 0, 1, 0, 0, 0, 1, 0),
    'f16_r32': (2, 0, 0, 0, 1, 0, 1, 0), 'f16_r32_stats': (2, 0, 0, 1, 1, 0, 1, 0),
    'f16_stream': (2, 0, 0, 0, 0, 0, 1, 1), 'f16_stream_stats': (2, 0, 0, 1, 0, 0, 1, 1),
}


def has_persistent_twin(form, tile=2):
    """has_persistent_twin of gemm.hip: the 256 x 256 tile, no fused rotary, no pair output, not the fp16 pair stream."""
    _, rotd, _, _, _, pair, _, rp = FORMS[form]
    return tile == 2 and rotd == 0 and not pair and not rp


PERSISTENT_FORMS = tuple(f for f in FORMS if has_persistent_twin(f))


def pick_tile(M, N, tile=0):
    """pick_tile of gemm.hip: 1 = 128 x 128, 2 = 256 x 256; 0 asks for the heuristic."""
    if tile:
        return tile
    return 2 if N >= 256 and ((M + 255) // 256) * ((N + 255) // 256) >= 160 else 1


def persist_default():
    """ESME_GEMM_PERSIST as the library reads it (once per process): on unless it is set to a number that is 0."""
    e = os.environ.get('ESME_GEMM_PERSIST')
    if e is None:
        return True
    m = re.match(r'\s*[+-]?\d+', e)                        # atoi: the leading integer, 0 where there is none
    return bool(m) and int(m.group()) != 0


def runs_persistent(form, M, N, tile, persist, vec_ok, ncu):
    """True where launch_one hands the call to the PERSIST = true instantiation.  `tile` 0 / 1 / 2 and `persist` -1 / 0 / 1 are the
    esme_gemm_opts_t fields (-1 follows ESME_GEMM_PERSIST), `vec_ok` the 16-byte epilogue of the call, `ncu` the device's compute units."""
    t = pick_tile(M, N, tile)
    if not has_persistent_twin(form, t):
        return False
    want = persist_default() if persist < 0 else persist != 0
    n = ncu & ~7
    return bool(want and vec_ok and n >= 8 and tile_counts(M, N)[0] * tile_counts(M, N)[1] >= 2 * n)


def grid(form, M, N, tile, persist, vec_ok, ncu):
    """Workgroups of the launch: one per compute unit (a multiple of 8) when persistent, else one per tile."""
    if runs_persistent(form, M, N, tile, persist, vec_ok, ncu):
        return ncu & ~7
    b = 128 * pick_tile(M, N, tile)
    return ((M + b - 1) // b) * ((N + b - 1) // b)


def tile_counts(M, N, b=256):
    return (M + b - 1) // b, (N + b - 1) // b


def raster(M, N, K, raster_gm=0, raster_gn=0, b=256):
    """set_raster of gemm.hip: (tiles_m, tiles_n, gm, gn)."""
    tm, tn = tile_counts(M, N, b)
    if raster_gm > 0:
        gm, gn = raster_gm, raster_gn if raster_gn > 0 else tn
    elif 2.0 * N * K <= 3.5e6 or tn <= 6:
        gm, gn = 1, tn
    elif tn % 5 == 0:
        gm, gn = 6, 5
    else:
        gm, gn = 8, 4
    return tm, tn, max(min(gm, tm), 1), max(min(gn, tn), 1)


def tile_coords(pid, tiles_m, tiles_n, gm, gn):
    """tile_coords of gemm_bf16_kernel: tile id -> (row tile, column tile).  Ids sweep bands of gm row tiles in groups of gn columns."""
    per_band = gm * tiles_n
    band, lb = divmod(pid, per_band)
    rows = min(gm, tiles_m - band * gm)
    ng, rg = divmod(lb, rows * gn)
    return band * gm + rg % rows, ng * gn + rg // rows


def walks(tiles, ncu):
    """The persistent kernel's split of the ids 0 .. tiles - 1 over ncu & ~7 workgroups: workgroup b serves XCD b & 7 as its slot b >> 3;
    XCD x owns the contiguous ids [base, end) (q = tiles >> 3 ids each, one more for the first r = tiles & 7), and a workgroup takes
    base + slot, base + slot + nslots, ... below end.  Returns (owner, position): per tile id, the workgroup and the tile's place in its walk."""
    n = ncu & ~7
    if n < 8:
        raise ValueError('the persistent kernel is never launched on fewer than 8 compute units')
    q, r, nslots = tiles >> 3, tiles & 7, n >> 3
    owner, position = [None] * tiles, [None] * tiles
    for b in range(n):
        xcd, slot = b & 7, b >> 3
        base = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
        end = base + q + (1 if xcd < r else 0)
        for step, pid in enumerate(range(base + slot, end, nslots)):
            assert owner[pid] is None, f'tile {pid} is walked twice'
            owner[pid], position[pid] = b, step
    return owner, position


def walk_positions(M, N, K, ncu, raster_gm=0, raster_gn=0):
    """(tiles_m, tiles_n) nested lists: the walk position of the tile at (row tile, column tile) in a persistent launch."""
    tm, tn, gm, gn = raster(M, N, K, raster_gm, raster_gn)
    _, position = walks(tm * tn, ncu)
    out = [[None] * tn for _ in range(tm)]
    for pid, p in enumerate(position):
        i, j = tile_coords(pid, tm, tn, gm, gn)
        assert out[i][j] is None
        out[i][j] = p
    return out


def kernel_name(form, tile, persistent):
    """The demangled instantiation as the launch log prints it."""
    epi, rotd, lnf, stats, r32, pair, f16, rp = FORMS[form]
    b = 'true' if persistent else 'false'
    t = lambda v: 'true' if v else 'false'
    dims = '256, 256, 2, 4' if tile == 2 else '128, 128, 2, 2'
    return f'esme::gemm_bf16_kernel<{dims}, {epi}, {rotd}, {t(lnf)}, {t(stats)}, {b}, {t(r32)}, {t(pair)}, {t(f16)}, {t(rp)}>(esme::GemmArgs)'
