"""The definition, the cases and a CPU emulation for the backward of the per-sequence mean (csrc/segment_mean_bwd.hip).

The kernel has one arithmetic step per element -- an IEEE fp32 division of a value that is exact in fp32 by an integer that is exact
in fp32 -- and one rounding, so its bound against the definition is ZERO: `expected` is `(dy.float() / len).to(dtype)` gathered per
row on the CPU (whose division is correctly rounded), zeros for the rows of no sequence, and `equal_bits` is the check.  `emulate`
walks the rows as the kernel does (bisection of cu_lens per row, a buffer that held NaN before) with switches for defects;
tests/test_segment_mean_bwd_cpu.py checks that the bit comparison accepts the faithful emulation and rejects each defect on the cases
tests/test_segment_mean_bwd_gpu.py runs.  Nothing here is tuned to a GPU run.
"""
import torch

ROWS = 32                      # ESME_HIP_SEGMENT_MEAN_BWD_ROWS (include/esme_hip_segment_mean_bwd.h)
LENGTHS = (0, 1, 2, 63, 64, 65, 129, 0, 200)   # empty sequences first and inside; around the 32-row tile and the 64-lane wave
START = 3                      # cu_lens[0]: rows before the first sequence
TAIL = 5                       # rows after the last sequence
ES = (8, 64, 1288)             # one 16-byte piece (bf16); a tile's pieces that fill whole waves; 161 pieces: a row straddles waves
DTYPES = (torch.bfloat16, torch.float32)
DEFECTS = ('wrong_length', 'next_row', 'no_zeroing', 'double_rounding')
CASES = [(f'{str(dt).split(".")[1]}-E{E}', dt, E) for dt in DTYPES for E in ES]


def cu_lens_of(lengths=LENGTHS, start=START):
    cu = torch.zeros(len(lengths) + 1, dtype=torch.int32)
    cu[0] = start
    cu[1:] = start + torch.cumsum(torch.tensor(lengths, dtype=torch.int32), 0) if len(lengths) else start
    return cu


def make_case(case, device='cpu', lengths=LENGTHS):
    """(dy (B, E), cu_lens int32 (B + 1), T): dy random with magnitudes over several binades (quotients by 63, 65, 129, 200 round)."""
    name, dtype, E = case
    g = torch.Generator().manual_seed(17 + E + (dtype == torch.float32))
    dy = (torch.randn(len(lengths), E, generator=g) * torch.exp2(torch.randint(-6, 7, (len(lengths), 1), generator=g).float())).to(dtype)
    cu = cu_lens_of(lengths)
    return dy.to(device), cu.to(device), int(cu[-1]) + TAIL


def expected(dy, cu_lens, T):
    """dX (T, E) in dy's dtype, on the CPU: (dy.float() / len).to(dtype) gathered per row; rows of no sequence are zeros."""
    dy, cu = dy.cpu(), cu_lens.cpu().long()
    lens = cu[1:] - cu[:-1]
    out = torch.zeros(T, dy.shape[1], dtype=dy.dtype)
    if lens.numel() == 0:
        return out
    g = (dy.float() / lens.clamp(min=1).float().view(-1, 1)).to(dy.dtype)
    seg = torch.repeat_interleave(torch.arange(lens.numel()), lens)
    a = int(cu[0])
    out[a:a + seg.numel()] = g[seg]
    return out


def bits(t):
    return t.cpu().contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def equal_bits(got, want):
    """The check: the same bit pattern in every element (a NaN left behind differs from a zero, -0 from +0)."""
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(bits(got), bits(want))


def defect_applies(defect, dtype):
    return dtype == torch.float32 if defect == 'double_rounding' else True


def emulate(dy, cu_lens, T, defect=None):
    """CPU emulation of esme_hip_segment_mean_bwd: dX (T, E) in a buffer that held NaN.  `defect`: None or one of DEFECTS --
    'wrong_length' (the divisor is cu_lens[s + 1] - cu_lens[0], the offset of the sequence's end instead of its length),
    'next_row' (a row takes the next non-empty sequence's dY when it is its sequence's last row: an off-by-one in the bisection),
    'no_zeroing' (rows of no sequence keep what the buffer held), 'double_rounding' (the quotient passes through bfloat16 before it
    is stored: shows for float32 only)."""
    assert defect is None or defect in DEFECTS, defect
    dy, cu = dy.cpu(), cu_lens.cpu().tolist()
    B, E = dy.shape
    out = torch.full((T, E), float('nan'), dtype=dy.dtype)
    y32 = dy.float()
    for r in range(T):
        lo, hi = 0, B + 1                                                  # the first index of cu[0 .. B] whose offset is > r
        while B > 0 and lo < hi:
            mid = (lo + hi) // 2
            bound = cu[mid] - 1 if (defect == 'next_row' and mid > 0) else cu[mid]
            if bound <= r:
                lo = mid + 1
            else:
                hi = mid
        s = lo - 1 if B > 0 else -1
        n = cu[s + 1] - cu[s] if 0 <= s < B else 0
        if n <= 0:
            if defect != 'no_zeroing':
                out[r] = 0
            continue
        if defect == 'wrong_length':
            n = cu[s + 1] - cu[0]
        q = y32[s] / torch.tensor(float(n), dtype=torch.float32)           # IEEE fp32
        if defect == 'double_rounding':
            q = q.to(torch.bfloat16).float()
        out[r] = q.to(dy.dtype)                                            # one rounding
    return out
