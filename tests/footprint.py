"""Where a kernel reads and writes: operands inside guard-banded arenas (used by test_footprint_cpu.py / test_footprint_gpu.py).

Every operand of a call is a view inside a larger tensor the test owns: GUARD_ROWS whole rows of the operand's row pitch before its
first and after its last row, and PAD_COLS pad columns on either side of every row (so ld > width and the operand's base is not the
allocation's base, though still 16-byte aligned).  A vector or a workspace is one row with the same pads; its row guards are capped at
VECTOR_GUARD_BYTES (256 KiB) on each side, still more than any tile can overhang.  The largest row tile / work item of the kernels is 256 rows, so nothing a tile
can overhang leaves the arena: a stray access lands in memory the test owns.  Guards and pads carry a recognisable fill, and
`check(case)` asserts

 1. write containment    every guard and pad byte of every operand, inputs included, is bit-identical to its fill after the call;
 2. read independence    the outputs are bit-identical between a run whose guards and pads are NaN (integer operands: a large
                         out-of-range value) and a run whose guards and pads are zero -- NaN, because a stray value that is
                         "masked" by a multiplication with 0 still shows;
 3. layout invariance    the outputs are bit-identical to the same call on plain contiguous tensors (what the float64-bound tests
                         vouch for); a case whose launcher legitimately picks another kernel for the arena's layout passes its own
                         comparison (`Case.plain_compare`) and says so;
 4. uninitialised workspaces   a 'ws' operand is exactly the number of bytes the size query returned, inside an arena, NaN-poisoned (0xFF bytes: a NaN at
                         every float width, the workspace and its guards alike) in one run and zeroed in the other: 2. then says no output depends on its previous contents and 1. that the
                         size query is large enough (`zeroed=True` where the header demands a zeroed workspace: only its guards are
                         poisoned).  'out' operands are poisoned the same way: an output element the call does not write shows.

What a green run does and does not prove:
 - it proves that no write lands outside an operand within the bands;
 - it proves that no value outside an operand, or in a workspace's previous contents, can reach an output through arithmetic;
 - it does NOT see a stray read whose value is discarded by a select, nor an access beyond the bands.

Operand extents are the ones include/esme_hip.h states, never what a kernel happens to touch.
"""
from __future__ import annotations

import dataclasses
from typing import Callable, Dict, List, Optional

import torch

GUARD_ROWS = 256          # rows of the operand's ld before and after it (the largest row tile / work item is 256 rows)
PAD_COLS = 64             # pad columns on each side of a row
VECTOR_GUARD_BYTES = 256 * 1024     # cap of the guard on each side of a 1-D operand (vectors, workspaces)

_FLOATS = (torch.bfloat16, torch.float16, torch.float32, torch.float64)
# integer operands (cu_lens, pos, idx, order, codes): a large out-of-range value in the 'nan' run
_INT_POISON = {1: 0x7F, 2: 0x3F3F, 4: 0x3F3F3F3F, 8: 0x3F3F3F3F3F3F3F3F}
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


@dataclasses.dataclass
class Operand:
    """One pointer argument.  `data`: CPU tensor, 1-D (a vector: one row) or 2-D (rows, cols): the case's contents ('out' / 'ws': shape
    and dtype only).  role: 'in', 'out' (every element written by the call: poisoned before it), 'inout' (read and / or partly
    written: holds `data`), 'ws' (a workspace: uint8 (nbytes)).  pad=False: the header fixes ld == width (a contiguous operand):
    guard rows only.  ld / lead: explicit row pitch and left pad in elements, for cases that need a particular pitch."""
    name: str
    data: torch.Tensor
    role: str = 'in'
    pad: bool = True
    ld: Optional[int] = None
    lead: Optional[int] = None
    zeroed: bool = False

    @property
    def rows(self):
        return 1 if self.data.dim() == 1 else self.data.shape[0]

    @property
    def cols(self):
        return self.data.shape[-1]


@dataclasses.dataclass
class Case:
    """`call(views)` runs the entry point on {operand name: view} (tensors of the operand's dtype and shape on the device; it takes
    pointers and row strides from them).  plain_compare(name, arena_out, plain_out): replaces the bit comparison of check 3 for a
    case whose launcher picks another kernel for another layout."""
    name: str
    operands: List[Operand]
    call: Callable[[Dict[str, torch.Tensor]], None]
    plain_compare: Optional[Callable] = None


class FootprintError(AssertionError):
    pass


def _poison(op, fill):
    es = op.data.element_size()
    if fill == 'zero':
        return 0
    if op.data.dtype in _FLOATS or op.role == 'ws':
        # all bits set: a NaN in bf16, fp16, fp32 and fp64, also when read at another width.  A workspace is raw bytes that the library
        # reads as floats: it and its guards get the same fill (0xFF bytes), never the finite integer poison
        return -1 if es > 1 else 0xFF
    return _INT_POISON[es]


def guard_rows(op, ld):
    """Rows of pitch `ld` before and after the operand.  2-D operands: GUARD_ROWS.  A vector or a workspace (one row, which no row tile
    can overhang by rows of ITS length): GUARD_ROWS rows too, but at most VECTOR_GUARD_BYTES on each side -- a workspace of several MB
    would otherwise cost GBs per run on machines shared with others -- and never less than one row."""
    if op.data.dim() != 1:
        return GUARD_ROWS
    return max(1, min(GUARD_ROWS, VECTOR_GUARD_BYTES // (ld * op.data.element_size())))


class Arena:
    """One operand inside its guard bands."""

    def __init__(self, op: Operand, fill: str, device):
        self.op = op
        dt = op.data.dtype
        self.es = es = op.data.element_size()
        self.idt = _INT_VIEW[es]
        rows, cols = op.rows, op.cols
        if op.pad:
            self.lead = PAD_COLS if op.lead is None else op.lead
            self.ld = op.ld if op.ld is not None else -(-(cols + 2 * PAD_COLS) // 16) * 16      # rows and base stay 16-byte aligned
        else:
            self.lead, self.ld = 0, cols
        assert self.ld >= self.lead + cols
        if op.pad and op.ld is None:
            assert self.lead >= PAD_COLS and self.ld - self.lead - cols >= PAD_COLS
        self.g = g = guard_rows(op, self.ld)
        self.buf = torch.full((rows + 2 * g, self.ld), _poison(op, fill), dtype=self.idt, device=device)
        inner = self.buf[g:g + rows, self.lead:self.lead + cols]
        if op.role in ('in', 'inout'):
            inner.copy_(op.data.reshape(rows, cols).contiguous().view(self.idt))
        elif op.role == 'ws' and op.zeroed:
            inner.zero_()
        typed = self.buf.view(dt)[g:g + rows, self.lead:self.lead + cols]
        self.view = typed[0] if op.data.dim() == 1 else typed
        self.before = self.buf.clone()

    def inner(self):
        return self.buf[self.g:self.g + self.op.rows, self.lead:self.lead + self.op.cols].clone().cpu()

    def violation(self) -> Optional[str]:
        """None, or a description of the guard / pad bytes that changed."""
        diff = self.buf != self.before
        diff[self.g:self.g + self.op.rows, self.lead:self.lead + self.op.cols] = False
        if not bool(diff.any()):
            return None
        a = self.buf.cpu().contiguous().view(torch.uint8)
        b = self.before.cpu().contiguous().view(torch.uint8)
        nbytes = int(((a != b) & diff.cpu().repeat_interleave(self.es, dim=1)).sum())
        pos = diff.cpu().nonzero()
        (r0, c0), (r1, c1) = pos[0].tolist(), pos[-1].tolist()
        return (f"operand '{self.op.name}' ({self.op.rows} x {self.op.cols} {self.op.data.dtype}, ld {self.ld}): {nbytes} bytes outside it were "
                f'written; first at (row {r0 - self.g}, col {c0 - self.lead}), last at (row {r1 - self.g}, col {c1 - self.lead}) '
                f'relative to the operand')


@dataclasses.dataclass
class Result:
    outputs: Dict[str, torch.Tensor]          # name -> integer (bit pattern) CPU tensor of every 'out' / 'inout' operand
    violations: List[str]


def _plain(op: Operand, device):
    """The operand as an ordinary contiguous tensor at the start of its allocation ('out' / 'ws': zeros, what a fresh test buffer usually
    holds), with the slack an allocator's rounding leaves behind it."""
    n = op.data.numel()
    buf = torch.zeros(n + 4096, dtype=op.data.dtype, device=device)
    if op.role in ('in', 'inout'):
        buf[:n].copy_(op.data.reshape(-1))
    return buf[:n].view(op.data.shape)


def _sync(device):
    if torch.device(device).type == 'cuda':
        torch.cuda.synchronize()


def run(case: Case, fill: str, device='cpu') -> Result:
    """Execute the case once.  fill: 'nan' / 'zero' (arenas with that guard fill) or 'plain' (contiguous tensors, no guards).  Every
    run builds fresh arenas, so in-place entry points start from the same contents."""
    if fill == 'plain':
        views = {op.name: _plain(op, device) for op in case.operands}
        case.call(views)
        _sync(device)
        return Result({op.name: views[op.name].cpu().view(_INT_VIEW[op.data.element_size()]).reshape(op.rows, op.cols)
                       for op in case.operands if op.role in ('out', 'inout')}, [])
    arenas = [Arena(op, fill, device) for op in case.operands]
    case.call({a.op.name: a.view for a in arenas})
    _sync(device)
    return Result({a.op.name: a.inner() for a in arenas if a.op.role in ('out', 'inout')},
                  [v for v in (a.violation() for a in arenas) if v is not None])


def _first_last(a, b):
    pos = (a != b).nonzero()
    return int((a != b).sum()), tuple(pos[0].tolist()), tuple(pos[-1].tolist())


def check(case: Case, device='cpu', plain=True) -> Dict[str, Result]:
    """The four checks of the module docstring; raises FootprintError naming the operand and the position."""
    res = {}
    for fill in ('nan', 'zero'):
        res[fill] = r = run(case, fill, device)
        if r.violations:
            raise FootprintError(f'{case.name} [{fill} guards]: write containment: ' + '; '.join(r.violations))
    for name, a in res['nan'].outputs.items():
        b = res['zero'].outputs[name]
        if not torch.equal(a, b):
            n, first, last = _first_last(a, b)
            raise FootprintError(f"{case.name}: read independence: output '{name}' depends on what lies outside the operands (or in a "
                                 f'workspace / output before the call): {n} elements differ between NaN and zero guards, first at (row {first[0]}, '
                                 f'col {first[1]}), last at (row {last[0]}, col {last[1]})')
    if plain:
        res['plain'] = p = run(case, 'plain', device)
        for name, a in res['nan'].outputs.items():
            b = p.outputs[name]
            if case.plain_compare is not None:
                case.plain_compare(name, a, b)
            elif not torch.equal(a, b):
                n, first, last = _first_last(a, b)
                raise FootprintError(f"{case.name}: layout invariance: output '{name}' differs from the call on contiguous tensors in {n} "
                                     f'elements, first at (row {first[0]}, col {first[1]}), last at (row {last[0]}, col {last[1]})')
    return res
