"""tests/gemm_path.py (which kernel a forward GEMM call runs) pinned against the launcher itself, and the coverage of the persistent kernels.

tools/kernel_launch_log.cpp --cases FILE runs the listed calls through the host side of csrc/gemm.hip on stubbed runtime symbols and prints
the launches.  The first test feeds it every shipped form under every tile / persist option on both sides of 2 * (compute units & ~7)
tiles at the harness's three devices (256, 4 and 300 compute units), with ESME_GEMM_PERSIST unset and 0, plus the vec_ok fallbacks, and
compares the instantiation (its PERSIST argument), the grid and the raster with gemm_path.  The second pushes the case table of
tests/test_gemm_persistent_bounds_gpu.py through it at 256 compute units: the PERSIST = true instantiations those cases launch must be
exactly the PERSIST = true symbols of the binary -- a persistent kernel without a float64-bound case fails here, as
tests/test_gemm_wgrad_gpu.py::test_both_paths_are_covered does for the weight-gradient paths.
"""
import re
import subprocess

import pytest

import gemm_path as gp
import gemm_persistent_cases as pc
from test_kernel_launch_log_cpu import KERNELS, _hipcc, build_harness, kernel_name

NCU = {0: 256, 1: 4, 2: 300}                               # compute units by the harness's device ordinal


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip('no hipcc in this environment')
    return build_harness(hipcc, str(tmp_path_factory.mktemp('kll')), 'gemm')


def run_cases(exe, rows, tmp_path, monkeypatch, persist_env=None):
    """rows of (form, M, N, K, tile, persist, gm, gn, device) -> per row the list of (kernel, grid, {field: value}) it launched."""
    path = tmp_path / 'cases.txt'
    path.write_text('# form M N K tile persist raster_gm raster_gn device\n' + ''.join(' '.join(str(v) for v in r) + '\n' for r in rows))
    if persist_env is None:
        monkeypatch.delenv('ESME_GEMM_PERSIST', raising=False)
    else:
        monkeypatch.setenv('ESME_GEMM_PERSIST', persist_env)
    out = subprocess.run([exe, '--cases', str(path)], check=True, capture_output=True, text=True).stdout
    blocks = re.split(r'^== line\d+ \d+\n', out, flags=re.M)[1:]
    assert len(blocks) == len(rows)
    got = []
    for b in blocks:
        launches = []
        for m in re.finditer(r'^launch (.*?\)) grid=(\d+),1,1 .*? (tiles_n=\d+ vec_ok=\d+) .*? (tiles_m=\d+ gm=\d+ gn=\d+) ', b, flags=re.M):
            fields = dict(kv.split('=') for kv in (m.group(3) + ' ' + m.group(4)).split())
            launches.append((kernel_name(m.group(1)), int(m.group(2)), {k: int(v) for k, v in fields.items()}))
        got.append(launches)
    return got


def pin_rows():
    rows = []
    for dev in NCU:
        for form in gp.FORMS:
            for tile in (0, 1, 2):
                for persist in (-1, 0, 1):
                    for tm in (170, 171, 197, 198):        # three tile columns: 510 / 513 tiles around 2 * 256, 591 / 594 around 2 * 296
                        rows.append((form, 256 * tm - 3, 768, 256, tile, persist, 0, 0, dev))
        for form in ('bf16_none', 'bf16_r32_stats', 'f16_gelu_ln', 'f16_stream', 'bf16_rot64'):
            for tm in (511, 512, 591, 592):                # one tile column: exactly one tile short of the threshold, and on it; a raster of its own
                rows.append((form, 256 * tm, 256, 64, 2, 1, 3, 4, dev))
                rows.append((form, 256 * tm, 256, 64, 2, -1, 0, 0, dev))
        for n in (516, 100):                               # N % 8 != 0: the scalar epilogue (vec_ok = 0) never persists
            rows.append(('bf16_gelu', 256 * 700, n, 128, 2, 1, 0, 0, dev))
        rows.append(('bf16_gelu', 256 * 700, 520, 128, 2, 1, 0, 0, dev))
    return rows


@pytest.mark.parametrize('persist_env', [None, '0', '1'])
def test_gemm_path_matches_the_launcher(harness, tmp_path, monkeypatch, persist_env):
    rows = pin_rows()
    got = run_cases(harness, rows, tmp_path, monkeypatch, persist_env)
    seen = set()
    for (form, M, N, K, tile, persist, gm, gn, dev), launches in zip(rows, got):
        vec_ok = N % 8 == 0                                # (the harness's buffers are aligned and ldc = N)
        what = f'{form} {M}x{N}x{K} tile {tile} persist {persist} raster {gm},{gn} on {NCU[dev]} compute units, ESME_GEMM_PERSIST={persist_env}'
        assert len(launches) == 1, what
        name, grid, f = launches[0]
        persistent = gp.runs_persistent(form, M, N, tile, persist, vec_ok, NCU[dev])
        t = gp.pick_tile(M, N, tile)
        assert name == gp.kernel_name(form, t, persistent), what
        assert grid == gp.grid(form, M, N, tile, persist, vec_ok, NCU[dev]), what
        if persistent:
            assert grid == NCU[dev] & ~7 and t == 2
        assert f['vec_ok'] == int(vec_ok), what
        assert (f['tiles_m'], f['tiles_n'], f['gm'], f['gn']) == gp.raster(M, N, K, gm, gn, 128 * t), what
        seen.add((dev, gp.has_persistent_twin(form), vec_ok, persistent))
    # both answers on every device that has a persistent launch, none on 4 compute units, and the fallbacks were there
    assert {(0, True, True, True), (0, True, True, False), (2, True, True, True), (2, True, True, False), (0, False, True, False),
            (0, True, False, False)} <= seen
    assert not any(p for d, _, _, p in seen if d == 1)


def test_env_switch_decides_option_minus_one(harness, tmp_path, monkeypatch):
    rows = [('bf16_none', 256 * 600, 256, 64, 2, p, 0, 0, 0) for p in (-1, 0, 1)]
    for env, want in ((None, [True, False, True]), ('0', [False, False, True]), ('2', [True, False, True])):
        got = run_cases(harness, rows, tmp_path, monkeypatch, env)
        assert [l[0][0] == gp.kernel_name('bf16_none', 2, True) for l in got] == want, env
        assert [gp.runs_persistent('bf16_none', 256 * 600, 256, 2, p, True, 256) for p in (-1, 0, 1)] == want, env


def test_every_persistent_kernel_has_a_float64_bound_case(harness, tmp_path, monkeypatch):
    """The case table of tests/test_gemm_persistent_bounds_gpu.py, at 256 compute units, launches all 17 PERSIST = true instantiations
    of the library and nothing but them."""
    table = pc.case_table()
    rows = [(form, *pc.shape(kind, form, 256), K, 2, 1, *raster, 0) for form, kind, K, raster in table]
    got = run_cases(harness, rows, tmp_path, monkeypatch)
    launched = set()
    for (form, kind, K, raster), row, launches in zip(table, rows, got):
        assert len(launches) == 1, row
        assert launches[0][0] == gp.kernel_name(form, 2, True) and launches[0][1] == 256, (row, launches)
        pc.assert_premise(form, kind, row[1], row[2], 256)
        launched.add(launches[0][0])
    symbols = subprocess.run(['nm', '-C', harness], check=True, capture_output=True, text=True).stdout.split('\n')
    built = {kernel_name(line.split(' ', 2)[2]) for line in symbols if re.search(KERNELS['gemm'][0], line)}
    assert len(built) == KERNELS['gemm'][1]
    persistent = {k for k in built if re.match(r'esme::gemm_bf16_kernel<(?:[^,]+, ){8}true,', k)}
    assert len(persistent) == 17 == len(gp.PERSISTENT_FORMS)
    assert launched == persistent, f'persistent kernels without a float64-bound case: {sorted(persistent - launched)}; launched but not built: {sorted(launched - persistent)}'
    # the shapes the GPU file uses below the threshold run the per-tile kernel
    less = [(form, *pc.shape('two_walks_less', form, 256), K, 2, 1, 0, 0, 0) for form in pc.SEAM_FORMS for K in pc.SEAM_K]
    for row, launches in zip(less, run_cases(harness, less, tmp_path, monkeypatch)):
        assert launches[0][0] == gp.kernel_name(row[0], 2, False) and launches[0][1] == 2 * 256 - 1, row
