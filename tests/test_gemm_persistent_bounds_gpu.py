"""The persistent 256 x 256 GEMM kernels -- all 17 PERSIST = true instantiations -- held to the per-element float64 bound at the tile seam.

Passing persist=1 does not force the persistent kernel: launch_one takes it from 2 * (compute units & ~7) tiles on (512 on an MI355X),
which no other float64-bound test reaches.  Every case here (tests/gemm_persistent_cases.py; shapes derived from the device's compute
units) therefore
  a) asserts through tests/gemm_path.py that its persist=1 call runs the persistent kernel, its persist=0 call the per-tile kernel, and
     that the walks have the lengths the shape is meant to give (positions 0, 1 and 2 present);
  b) hands over C and stats_out full of NaN (the fp32 stream is updated in place: an unwritten tile keeps the old stream and misses c);
  c) holds every output of the persistent kernel to error_bounds.assert_bounded with the recipe and operands of the matching test of
     tests/test_error_bounds_gpu.py, unchanged, and takes the rounding bias where the recipe leaves elements for it;
  d) asserts the bits of the per-tile kernel: C, the statistics rows, the fp32 stream;
  e) records the worst err / bound per walk position (0, 1, >= 2): a seam defect shows as a jump from position 1 on, and a failure
     message names the walk position beside the tile.
tests/test_gemm_persistent_cpu.py shows on an emulation that these checks reject six seam defects; tests/test_gemm_path_cpu.py that the
table reaches every persistent instantiation.  The tables are printed at the end of the module (run with -s): profiles/gemm_persistent_bounds.txt.
"""
import time

import pytest
import torch

import gemm_operands as ops
import gemm_path as gp
import gemm_persistent_cases as pc
from esme import _hip

pytestmark = pytest.mark.gpu
LEDGER = ops.Ledger('persistent gemm')
POSITIONS = {}                                             # (form, result, output) -> worst err / bound at walk position 0, 1, >= 2


def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count & ~7


@pytest.fixture(scope='module', autouse=True)
def _report():
    t0 = time.time()
    yield
    LEDGER.report()
    print('[persistent gemm] worst err / bound per walk position (0, 1, >= 2); the per-tile kernel writes the same tiles with no seam:')
    for k in sorted(POSITIONS):
        print(f'  {k[0]:18s} {k[1]:10s} {k[2]:4s} ' + ' '.join(f'{v:6.3f}' for v in POSITIONS[k]))
    print(f'[persistent gemm] {ncu()} persistent workgroups; wall time of the file {time.time() - t0:.1f} s')


def run_case(form, kind, K):
    n = ncu()
    M, N = pc.shape(kind, form, n)
    pc.assert_premise(form, kind, M, N, n)
    o = pc.operands(form, M, N, K, hip=_hip)
    got_p, got_t = pc.launch(o, _hip, 1), pc.launch(o, _hip, 0)
    tables = pc.hold(f'{form} {kind} {M}x{N}x{K}', o, got_p, got_t, n, ledger=LEDGER)
    for tag, table in tables.items():
        for name, row in table.items():
            prev = POSITIONS.get((form, tag, name), [0.0, 0.0, 0.0])
            POSITIONS[(form, tag, name)] = [max(a, b) for a, b in zip(prev, row)]
    return o, got_p


@pytest.mark.parametrize('K', pc.BASE_K)
@pytest.mark.parametrize('form', pc.FORMS)
def test_persistent_form_meets_the_float64_bound(form, K):
    """The smallest launch with walks of different lengths (one more tile than two walks, three tile columns, the last 8 columns wide, the
    last row tile one row deep), at 1, 2, 3 and 5 K-tiles."""
    run_case(form, 'base', K)


@pytest.mark.parametrize('K', pc.SEAM_K)
@pytest.mark.parametrize('kind', pc.SEAM_SHAPES)
@pytest.mark.parametrize('form', pc.SEAM_FORMS)
def test_persistent_walk_lengths(form, kind, K):
    """Exactly two walks per workgroup; 2 ncu + 7 tiles (XCD ranges of unequal length); three tiles and more for every workgroup."""
    run_case(form, kind, K)
    if kind == 'two_walks':                                # one tile fewer, and the launcher leaves the persistent kernel
        n = ncu()
        M, N = pc.shape('two_walks_less', form, n)
        assert not gp.runs_persistent(form, M, N, 2, 1, True, n) and gp.grid(form, M, N, 2, 1, True, n) == 2 * n - 1
        o = pc.operands(form, M, N, K, hip=_hip)
        got = pc.launch(o, _hip, 1)
        pc.check_written(f'{form} {M}x{N}x{K} per tile', got)
        pc.check_bounded(f'{form} {M}x{N}x{K}', o, got, n, ledger=LEDGER, tag='per tile')


@pytest.mark.parametrize('form', pc.SEAM_FORMS)
def test_persistent_rasters_bit_equal(form):
    """The six (gm, gn) groupings of test_gemm_options_bit_equal walked by the persistent kernel: the same bits as the default walk."""
    n = ncu()
    M, N = pc.shape('base', form, n)
    pc.assert_premise(form, 'base', M, N, n)                # (the raster moves tiles between walks, not the launch off the persistent kernel)
    o = pc.operands(form, M, N, pc.RASTER_K, hip=_hip)
    base = pc.launch(o, _hip, 1, pc.RASTERS[0])
    pc.check_written(f'{form} raster {pc.RASTERS[0]}', base)
    for raster in pc.RASTERS[1:]:
        got = pc.launch(o, _hip, 1, raster)
        pc.check_written(f'{form} raster {raster}', got)
        for name in base:
            assert torch.equal(got[name], base[name]), f'{form}: {name} under raster {raster} differs from the default walk'
