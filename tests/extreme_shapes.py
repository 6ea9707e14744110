"""Shared inputs and comparators for the tests past the launch limits of the training and observer kernels
(tests/test_extreme_shapes_train_gpu.py on the device, tests/test_extreme_shapes_train_cpu.py for the comparators themselves).

Two limits are meant.  A kernel that takes the sequence from grid z runs in launches of at most GRID_Z = 65 535 sequences and
indexes with `b0 + blockIdx.z`: a batch of more than 65 535 sequences is the only input on which the second launch runs.  And a row
offset `row * ld` passes 2^31 elements either between sequences (a 64-bit product) or inside one sequence (an unsigned 32-bit
product, valid to 2^32): a row stride of 2^20 elements puts both within reach of a buffer that fits the device.

torch and numpy only: no device, no library.  The checks are written over flat tensors and element ranges, so one function serves
packed rows (ranges from cu_lens) and packed maps (ranges from map offsets), and the batch constant is a parameter: the CPU file runs
the same functions on a reduced batch with a reduced `grid_z`.
"""
import numpy as np
import torch

GRID_Z = 65535
SPLIT = 40000                     # the two sub-batches [0, SPLIT) and [SPLIT, B): each is one launch


# ------------------------------------------------------------------ batches

def many_lengths(seed=0):
    """test_extreme_shapes_gpu.many_lengths: 70 000 sequences of 1 to 8 residues between two of 300 (B = 70 002)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [300] + rng.integers(1, 9, size=70000).tolist() + [300]


def row_lengths(seed=1, B=70002):
    """B sequences of 0 to 12 rows, for the row kernels: empty sequences included, on both sides of sequence 65 535."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(0, 13, size=B).tolist()


def cu_of(lengths, start=0):
    cu = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    cu[1:] = torch.tensor(lengths, dtype=torch.int64).cumsum(0)
    return (cu + start).to(torch.int32)


def picks(B, grid_z=GRID_Z, seed=7, extra=40):
    """The sequences that get the float64 comparison: both ends, grid_z - 2 .. grid_z + 5 (the last sequences of the first launch and
    the first of the second) and `extra` seeded indices."""
    rng = np.random.Generator(np.random.PCG64(seed))
    fixed = {0, 1, B - 1} | set(range(grid_z - 2, grid_z + 6))
    assert all(0 <= i < B for i in fixed), (B, grid_z)
    return sorted(fixed | set(rng.integers(0, B, size=extra).tolist()))


def halves(B, split=SPLIT):
    return [(0, split), (split, B)]


def ranges_index(starts, sizes, which):
    """int64 index of the elements [starts[i], starts[i] + sizes[i]) for i in `which`, in that order."""
    parts = [torch.arange(int(starts[i]), int(starts[i]) + int(sizes[i])) for i in which]
    return torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64)


def sub_batch(x, cu, which):
    """(the rows of the sequences `which` of every tensor in x, their cu_lens int32).  x: one (T, ...) tensor or a tuple of them."""
    cul = cu.tolist() if isinstance(cu, torch.Tensor) else list(cu)
    lens = [cul[i + 1] - cul[i] for i in which]
    rows = ranges_index(cul, [b - a for a, b in zip(cul[:-1], cul[1:])], which)
    take = lambda t: t[rows.to(t.device)].contiguous()
    return (tuple(take(t) for t in x) if isinstance(x, (tuple, list)) else take(x)), cu_of(lens)


# ------------------------------------------------------------------ buffers past 2^31

def wide_buffer(rows, ld, dtype, device):
    """(rows, ld) over one uninitialised allocation: operands are column blocks of it, so every one of them has the row stride ld."""
    assert rows * ld > 1 << 31
    return torch.empty(rows * ld, dtype=dtype, device=device).view(rows, ld)


def crossing(lengths, ld):
    """What of a packed batch lies at an element offset >= 2^31 of a buffer with row stride ld:
    `first_row` the first such packed row, `sequences` those that start there, `inside` (s, first in-sequence row) of the sequences
    whose own rows reach an offset >= 2^31 from the sequence's first row (where a signed 32-bit product would be wrong)."""
    first_row = -(-(1 << 31) // ld)
    starts = np.concatenate(([0], np.cumsum(lengths)))
    T = int(starts[-1])
    sequences = [s for s, n in enumerate(lengths) if n and starts[s] >= first_row]
    inside = [(s, first_row) for s, n in enumerate(lengths) if n > first_row]
    assert first_row < T and (sequences or inside), f'nothing of {T} rows x {ld} lies past 2^31 elements'
    assert max(lengths) * ld < 1 << 32, 'a sequence passes 2^32 elements: outside what the kernels accept'
    return dict(first_row=first_row, sequences=sequences, inside=inside)


# ------------------------------------------------------------------ comparators

def _bits(t):
    t = t.detach().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_rows_equal(got, want, what):
    """Bit equality (a NaN left behind differs from a value, -0 from +0)."""
    assert got.shape == want.shape and got.dtype == want.dtype, f'{what}: {tuple(got.shape)} {got.dtype} against {tuple(want.shape)} {want.dtype}'
    a, b = _bits(got), _bits(want.to(got.device))
    if not torch.equal(a, b):
        bad = (a != b).reshape(a.shape[0], -1).any(1).nonzero().reshape(-1)
        raise AssertionError(f'{what}: {bad.numel()} of {a.shape[0]} rows differ, the first at {int(bad[0])}, the last at {int(bad[-1])}')


def assert_inside(got, ref, bound, what):
    """max |got - ref| / bound <= 1.0 and every value finite (an exact match on a zero bound counts as 0).  Tensors, or equally long
    sequences of tensors.  Prints and returns the worst ratio."""
    if isinstance(got, torch.Tensor):
        got, ref, bound = [got], [ref], [bound]
    assert len(got) == len(ref) == len(bound), what
    worst = 0.0
    for i, (g, r, b) in enumerate(zip(got, ref, bound)):
        assert tuple(g.shape) == tuple(r.shape) == tuple(b.shape), f'{what}: part {i}: shapes {tuple(g.shape)} / {tuple(r.shape)} / {tuple(b.shape)}'
        if not g.numel():
            continue
        g64 = g.detach().double()
        assert bool(torch.isfinite(g64).all()), f'{what}: part {i}: non-finite values'
        err = (g64 - r.to(g64.device).double()).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / b.to(g64.device).double())
        worst = max(worst, float(ratio.max()))
    print(f'{what}: worst err / bound {worst:.3f}')
    assert worst <= 1.0, f'{what}: worst err / bound {worst:.3g}'
    return worst


# ------------------------------------------------------------------ the checks of a batch past grid_z sequences

def assert_split_identity(full, starts, run_part, B, what, split=SPLIT):
    """Every sequence of the full run is bit-equal to the same sequence run inside [0, split) or [split, B).  `full`: the full run's
    output, flat or in rows; `starts` (B + 1): where each sequence's elements begin in it; run_part(a, b): the output of the
    sub-batch of sequences a .. b - 1, laid out the same way."""
    for a, b in halves(B, split):
        part = run_part(a, b)
        lo, hi = int(starts[a]), int(starts[b])
        assert part.shape[0] == hi - lo, f'{what}: sub-batch [{a}, {b}) has {part.shape[0]} elements, the full run {hi - lo}'
        assert_rows_equal(full[lo:hi], part, f'{what}: sequences [{a}, {b}) packed in the whole batch against the sub-batch')


def assert_picks_identity(full, starts, alone, which, what):
    """The picked sequences' elements of the full run are bit-equal to `alone`, the output of the picks run as a batch of their own."""
    sizes = [int(starts[i + 1]) - int(starts[i]) for i in range(len(starts) - 1)]
    idx = ranges_index(starts, sizes, which).to(full.device)
    assert_rows_equal(full[idx], alone, f'{what}: the picks packed in the whole batch against the picks alone')


# ------------------------------------------------------------------ untouched surroundings

def assert_untouched(buf, fill_bits, rows, cols, what, chunk=4096):
    """Every element of the 2-D `buf` outside rows [rows[0], rows[1]) x the column ranges `cols` still holds the bit pattern `fill_bits`
    (buf was filled through its integer view).  Walks row chunks so that no temporary of the buffer's size is made."""
    bits = buf.view({2: torch.int16, 4: torch.int32}[buf.element_size()])
    cols = sorted(cols)
    for r0 in range(0, bits.shape[0], chunk):
        r1 = min(r0 + chunk, bits.shape[0])
        a, b = min(max(rows[0], r0), r1), min(max(rows[1], r0), r1)         # the chunk's rows [a, b) hold operands
        for lo, hi in ((r0, a), (b, r1)):
            if lo < hi:
                assert bool((bits[lo:hi] == fill_bits).all()), f'{what}: rows {lo} .. {hi - 1} outside the operands were written'
        if a < b:
            edge = 0
            for c0, c1 in cols + [(bits.shape[1], bits.shape[1])]:
                if edge < c0:
                    assert bool((bits[a:b, edge:c0] == fill_bits).all()), f'{what}: columns {edge} .. {c0 - 1} of rows {a} .. {b - 1} were written'
                edge = max(edge, c1)
