"""The launch sequence of the one-call forwards (csrc/forward.hip), checked on the CPU.

forward.hip is host-only code.  tools/forward_launch_log.cpp links it against logging stubs of the 18 entries it calls and runs a table
of descriptors (fast / half / exact; ESM-2 at head dims 16 .. 128, ESM-C, ESM-1b, a padded layout; extension tile, q / k pairs, guards,
LM head, refusals) through the three entries.  tests/golden/forward_launch_log.txt holds, per case, the number of launches and the sha256
of the log: every entry, scalar, normalised pointer and fusion field.  A host-side change to forward.hip must leave every line as it is;
regenerate the golden (tools/README.md) only for a change that is MEANT to alter a launch.

    python tests/test_forward_launch_log_cpu.py [path/to/forward.hip]      prints the golden lines for that source
"""
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'esm-efficient_amd', 'csrc')
HARNESS = os.path.join(ROOT, 'tools', 'forward_launch_log.cpp')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'forward_launch_log.txt')


def _hipcc():
    return shutil.which('hipcc') or (os.path.exists('/opt/rocm/bin/hipcc') and '/opt/rocm/bin/hipcc') or None


def build_harness(hipcc, out_dir, forward_hip=None, extra=()):
    """Host-only build of the harness against `forward_hip` (default: the tree's); returns the executable."""
    exe = os.path.join(out_dir, 'forward_launch_log')
    cmd = [hipcc, '--offload-host-only', '-std=c++17', '-O1', '-I', CSRC, *extra, '-o', exe, HARNESS, forward_hip or os.path.join(CSRC, 'forward.hip')]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-4000:]
    return exe


def digest_lines(exe):
    """'name calls sha256' per case, from the harness's full output ('== name calls' opens a case)."""
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    lines = []
    for block in out.split('== ')[1:]:
        head, _, log = block.partition('\n')
        name, calls = head.split()
        lines.append(f'{name} {calls} {hashlib.sha256(log.encode()).hexdigest()}')
    return lines


def test_forward_launch_log_matches_golden(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip('no hipcc in this environment')
    got = digest_lines(build_harness(hipcc, str(tmp_path)))
    want = open(GOLDEN).read().split('\n')[:-1]
    assert len(want) >= 80 and len({line.split()[0] for line in want}) == len(want)
    assert [line.split()[0] for line in got] == [line.split()[0] for line in want], 'the case table and the golden list different cases'
    wrong = [f'{g}   (golden: {w})' for g, w in zip(got, want) if g != w]
    assert not wrong, 'launch logs differ (diff `forward_launch_log --dump CASE` against a build with the previous forward.hip):\n' + '\n'.join(wrong)


if __name__ == '__main__':
    with tempfile.TemporaryDirectory() as td:
        print('\n'.join(digest_lines(build_harness(_hipcc(), td, sys.argv[1] if len(sys.argv) > 1 else None))))
