"""Which kernel a GEMM or attention call launches (csrc/gemm.hip, csrc/attn.hip), checked on the CPU.

tools/kernel_launch_log.cpp includes the host side of one of the two sources, stubs the HIP runtime symbols it touches and runs a table
of calls on fake pointers through every C entry: all 38 GEMM forms under both tiles and the heuristic, persistence at three compute-unit
counts, every raster arm, the vec_ok fallbacks, the column split, the attention entries over head dims / lengths / variants / fp16 /
prescaled q, more than 65 535 sequences, and every refusal (alone and in pairs, which fixes the precedence of the messages).
tests/golden/kernel_launch_log.txt holds, per case, the number of launches and the sha256 of the log: kernel instantiation, grid, block,
dynamic LDS and every field of the argument struct.  The GEMM harness runs twice (ESME_GEMM_PERSIST unset and =0; read once per process).
A host-side change must leave every line as it is; regenerate the golden (tools/README.md) only for a change that is MEANT to alter a launch.

    python tests/test_kernel_launch_log_cpu.py [path/to/gemm.hip | path/to/attn.hip]     prints the golden lines (default: both, the tree's)
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'esm-efficient_amd', 'csrc')
HARNESS = os.path.join(ROOT, 'tools', 'kernel_launch_log.cpp')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'kernel_launch_log.txt')
KERNELS = {'gemm': (r'gemm_bf16_kernel<', 93), 'attn': (r'attn_\w+_kernel<', 38)}     # instantiations of the shipped library


def _hipcc():
    return shutil.which('hipcc') or (os.path.exists('/opt/rocm/bin/hipcc') and '/opt/rocm/bin/hipcc') or None


def build_harness(hipcc, out_dir, which, source=None, extra=()):
    """Host-only build of the harness around `source` (default: the tree's gemm.hip / attn.hip); returns the executable."""
    exe = os.path.join(out_dir, 'kernel_launch_log_' + which)
    source = os.path.abspath(source or os.path.join(CSRC, which + '.hip'))
    cmd = [hipcc, '--offload-host-only', '-std=c++17', '-O1', '-rdynamic', '-Wl,--unresolved-symbols=ignore-all', '-I', os.path.join(ROOT, 'include'),
           '-I', CSRC, '-DESME_KLL_' + which.upper(), f'-DESME_SRC="{source}"', *extra, '-o', exe, '-x', 'hip', HARNESS, os.path.join(CSRC, 'api.hip'), '-ldl']
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-4000:]
    return exe


def run_harness(exe, persist=None):
    env = {k: v for k, v in os.environ.items() if k != 'ESME_GEMM_PERSIST'}
    if persist is not None:
        env['ESME_GEMM_PERSIST'] = persist
    return subprocess.run([exe], check=True, capture_output=True, text=True, env=env).stdout


def digest_lines(out, prefix):
    """'prefix:name launches sha256' per case, from the harness's full output ('== name launches' opens a case)."""
    lines = []
    for block in re.split(r'^== ', out, flags=re.M)[1:]:
        head, _, log = block.partition('\n')
        name, launches = head.split()
        lines.append(f'{prefix}:{name} {launches} {hashlib.sha256(log.encode()).hexdigest()}')
    return lines


def golden_lines(hipcc, out_dir, which, source=None):
    """(lines, executable, concatenated output) of one source: gemm twice (ESME_GEMM_PERSIST unset, =0), attn once."""
    exe = build_harness(hipcc, out_dir, which, source)
    out = run_harness(exe)
    lines = digest_lines(out, which)
    if which == 'gemm':
        out0 = run_harness(exe, persist='0')
        lines += digest_lines(out0, 'gemm_persist0')
        out += out0
    return lines, exe, out


def kernel_name(text):
    return text.replace('__device_stub__', '').replace('void ', '', 1).strip()


@pytest.mark.parametrize('which', ['gemm', 'attn'])
def test_kernel_launch_log_matches_golden(which, tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip('no hipcc in this environment')
    got, exe, out = golden_lines(hipcc, str(tmp_path), which)
    want = [line for line in open(GOLDEN).read().split('\n')[:-1] if line.split(':')[0].startswith(which)]
    assert len(want) >= 200 and len({line.split()[0] for line in want}) == len(want)
    assert [line.split()[0] for line in got] == [line.split()[0] for line in want], 'the case table and the golden list different cases'
    wrong = [f'{g}   (golden: {w})' for g, w in zip(got, want) if g != w]
    assert not wrong, 'launch logs differ (diff `kernel_launch_log --dump CASE` against a build with the previous source):\n' + '\n'.join(wrong)
    # every instantiation the source holds is launched by some case, and nothing else is: the refactored launcher instantiates what the
    # previous one did (93 GEMM and 38 attention kernels), no more and no fewer
    pattern, count = KERNELS[which]
    symbols = subprocess.run(['nm', '-C', exe], check=True, capture_output=True, text=True).stdout.split('\n')
    built = {kernel_name(line.split(' ', 2)[2]) for line in symbols if re.search(pattern, line)}
    launched = {kernel_name(m) for m in re.findall(r'^launch (.*?\)) grid=', out, flags=re.M)}
    assert launched == built, f'never launched: {sorted(built - launched)}; launched but not a symbol: {sorted(launched - built)}'
    assert len(built) == count


if __name__ == '__main__':
    sources = sys.argv[1:] or [os.path.join(CSRC, 'gemm.hip'), os.path.join(CSRC, 'attn.hip')]
    with tempfile.TemporaryDirectory() as td:
        for src in sources:
            which = 'gemm' if 'gemm' in os.path.basename(src) else 'attn'
            print('\n'.join(golden_lines(_hipcc(), td, which, src)[0]))
