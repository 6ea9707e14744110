"""Where a non-finite operand VALUE may go: used by test_nonfinite_cpu.py / test_nonfinite_gpu.py.

tests/footprint.py poisons the bytes AROUND an operand.  This harness poisons values INSIDE it: the rows of one sequence of a packed
batch, the columns of one head, one row, one tensor of a list.  A `Case` is a call on CPU tensors (the operands of footprint.Operand, run
on plain contiguous device tensors) with a list of `Unit`s; a unit names the region of each floating input to poison and the region of
each output that may depend on it.  `check(case)` runs the call once clean and once per (unit, operand, poison) -- every float operand
of the unit alone, then all together -- and asserts

 1. clean run      every floating output is finite;
 2. containment    outside the unit's output region every output is bit-identical to the clean run (integer view): a tail tile that
                   reads a neighbour's rows "times zero" shows, because 0 * NaN and 0 * Inf are NaN;
 3. propagation    inside the region the output is never finite where the truth is not: NaN in gives NaN out; for +-Inf the expected
                   class comes from LIMITS, the extended-real limits of the operation (NaN is accepted wherever a limit exists: torch
                   gives gelu(-inf) = nan where the kernel's formula gives the exact limit 0).  A finite value where the limit is
                   infinite or undefined is the failure.

Poisons: all-ones bits (footprint._poison: a NaN at every float width), +Inf, and -Inf where the case lists it (neg_inf=True).
Outputs that reduce over all sequences by design (weight and bias gradients, d_table, d_pos, dU, grad_sqnorm, col_absmax, qk_sumsq) are
named in Case.reduced: no containment check.  Exceptions to 3. live in KNOWN_SWALLOWS, each quoting the kernel comment that justifies it;
for such a case only the propagation check is skipped.  The table may not grow without a comment of the same kind in the kernel.
"""
from __future__ import annotations

import dataclasses
from typing import Callable, Dict, List, Optional, Tuple

import torch

import footprint as fp
from footprint import Operand          # noqa: F401  (re-exported: cases are written with it)

_INT_VIEW = fp._INT_VIEW
POISONS = ('nan', '+inf', '-inf')

# The extended-real limit of an operation at an infinite operand: 'nonfinite' (the limit is infinite, or undefined as in inf - inf and
# 0 * inf: a finite output is the failure) or 'any' (a finite limit exists: finite or NaN are both accepted).  NaN in is always NaN out.
LIMITS = {
    'linear': {'+inf': 'nonfinite', '-inf': 'nonfinite'},        # sums of products, normalisations, softmax over a poisoned row
    'relu': {'+inf': 'nonfinite', '-inf': 'any'},                # relu(+inf) = +inf, relu(-inf) = 0
    'gelu': {'+inf': 'nonfinite', '-inf': 'any'},                # gelu(+inf) = +inf, gelu(-inf) = 0
    'score': {'+inf': 'nonfinite', '-inf': 'any'},               # a -inf score gives softmax weight 0
}

KNOWN_SWALLOWS = {
    'gelu_deg5_ln_fold': (
        'esm-efficient_amd/csrc/common.h:211-215',
        "NaN: v_min / v_max return their non-NaN operand, so the formula maps NaN to 0. [...] the degree-5 site (the LayerNorm-folded FFN "
        "up-projection, where every VALU instruction costs 0.2 ms per step) keeps the bare formula: a NaN there comes from a non-finite "
        "residual stream, which the run-time range guard reports (esme_gemm_fusion_t.overflow_flag) and which reaches the output through "
        "the attention branch anyway."),
}

Region = Tuple[object, object]          # (rows, cols): None (all), an int, a slice, or a list / 1-D tensor of indices


class NonFiniteError(AssertionError):
    pass


@dataclasses.dataclass
class Unit:
    """poison: {float input operand: region to poison}, or {label: (operand, rows, cols)} where several parts of one tensor are operands of
    their own (q, k and v as column blocks of one buffer).  affects: {output: region that MAY depend on it} (an output not named may
    not depend on it at all).  must: {output: region whose true value is non-finite}; default: `affects`.  together_only: skip the runs
    with one operand poisoned alone (they are units of their own, with their own `must`)."""
    name: str
    poison: Dict[str, Region]
    affects: Dict[str, Region]
    must: Optional[Dict[str, Region]] = None
    together_only: bool = False


@dataclasses.dataclass
class Case:
    """call(views): as footprint.Case.  op: the LIMITS row of the operation, or {operand: row} where operands differ.  reduced: outputs that
    reduce over all units by design.  swallow: a KNOWN_SWALLOWS key."""
    name: str
    operands: List[Operand]
    call: Callable[[Dict[str, torch.Tensor]], None]
    units: List[Unit]
    op: object = 'linear'
    neg_inf: bool = False
    reduced: Tuple[str, ...] = ()
    swallow: Optional[str] = None

    @classmethod
    def of(cls, fcase: fp.Case, units, **kw):
        """From a footprint case: the same operands and call."""
        return cls(fcase.name, fcase.operands, fcase.call, units, **kw)


def _index(i, n):
    if i is None:
        return torch.arange(n)
    if isinstance(i, int):
        return torch.tensor([i % n if n else 0])
    if isinstance(i, slice):
        return torch.arange(n)[i]
    return torch.as_tensor(i, dtype=torch.long).reshape(-1)


def region_mask(region: Region, rows: int, cols: int) -> torch.Tensor:
    m = torch.zeros(rows, cols, dtype=torch.bool)
    r, c = _index(region[0], rows), _index(region[1], cols)
    if r.numel() and c.numel():
        m[r[:, None], c[None, :]] = True
    return m


def poison_value(kind: str, dtype):
    """The poison as the integer bit pattern of `dtype`."""
    idt = _INT_VIEW[torch.empty(0, dtype=dtype).element_size()]
    if kind == 'nan':
        return torch.tensor(-1, dtype=idt)                       # all bits set, as footprint._poison
    return torch.tensor(float('inf') if kind == '+inf' else float('-inf'), dtype=dtype).view(idt)


def _device_operand(op: Operand, device, poison):
    n = op.data.numel()
    if op.role in ('in', 'inout'):
        data = op.data.reshape(op.rows, op.cols).clone() if n else op.data.clone()
        for region, kind in (poison if n else ()):
            assert data.dtype.is_floating_point, f"operand '{op.name}' is not floating point"
            bits = data.view(_INT_VIEW[data.element_size()])
            bits[region_mask(region, op.rows, op.cols)] = poison_value(kind, data.dtype)
        buf = torch.zeros(n + 4096, dtype=op.data.dtype, device=device)          # (the slack an allocator's rounding leaves, as footprint._plain)
        buf[:n].copy_(data.reshape(-1))
    else:
        buf = torch.zeros(n + 4096, dtype=op.data.dtype, device=device)
    return buf[:n].view(op.data.shape)


def _resolve(label, value):
    """(operand, region) of one entry of Unit.poison."""
    return (value[0], (value[1], value[2])) if len(value) == 3 else (label, value)


def run(case: Case, device='cpu', poison: Optional[Dict[str, tuple]] = None) -> Dict[str, torch.Tensor]:
    """One execution on fresh contiguous tensors; {output: integer (bit pattern) CPU tensor (rows, cols)} of every 'out' / 'inout' operand.
    poison: {label: (region or (operand, rows, cols), kind)}."""
    todo = {}
    for label, (value, kind) in (poison or {}).items():
        name, region = _resolve(label, value)
        todo.setdefault(name, []).append((region, kind))
    views = {op.name: _device_operand(op, device, todo.get(op.name, ())) for op in case.operands}
    case.call(views)
    fp._sync(device)
    return {op.name: views[op.name].cpu().contiguous().view(_INT_VIEW[op.data.element_size()]).reshape(op.rows, op.cols)
            for op in case.operands if op.role in ('out', 'inout') and op.data.numel()}


def _where(mask):
    pos = mask.nonzero()
    return int(mask.sum()), tuple(pos[0].tolist()), tuple(pos[-1].tolist())


def _limit(case, operand, kind):
    if kind == 'nan':
        return 'nan'
    op = case.op.get(operand, 'linear') if isinstance(case.op, dict) else case.op
    return LIMITS[op][kind]


def check(case: Case, device='cpu') -> Dict[str, int]:
    """The three checks of the module docstring; raises NonFiniteError naming the check, the unit, the operand, the poison and the first /
    last offending (row, col).  Returns {'units', 'poisons' (poisoned runs), 'swallows' (KNOWN_SWALLOWS entries used)}."""
    if case.swallow is not None:
        assert case.swallow in KNOWN_SWALLOWS, case.swallow
    ops = {op.name: op for op in case.operands}
    clean = run(case, device)
    for name, bits in clean.items():
        dt = ops[name].data.dtype
        if dt.is_floating_point:
            bad = ~torch.isfinite(bits.view(dt).float())
            if bool(bad.any()):
                n, first, last = _where(bad)
                raise NonFiniteError(f"{case.name}: clean run: output '{name}' holds {n} non-finite values, first at (row {first[0]}, col {first[1]}), "
                                     f'last at (row {last[0]}, col {last[1]})')
    kinds = [k for k in POISONS if k != '-inf' or case.neg_inf]
    runs = 0
    for unit in case.units:
        names = list(unit.poison)
        for n in names:
            o = ops[_resolve(n, unit.poison[n])[0]]
            assert o.role in ('in', 'inout') and o.data.dtype.is_floating_point, f'{case.name}: {n} is no floating input'
        groups = ([] if unit.together_only else [[n] for n in names]) + ([names] if len(names) > 1 or unit.together_only else [])
        for group in groups:
            for kind in kinds:
                got = run(case, device, {n: (unit.poison[n], kind) for n in group})
                runs += 1
                what = f"{case.name}: unit '{unit.name}', operand {' + '.join(group)}, poison {kind}"
                for name, bits in got.items():
                    op = ops[name]
                    inside = region_mask(unit.affects[name], op.rows, op.cols) if name in unit.affects else torch.zeros(op.rows, op.cols, dtype=torch.bool)
                    if name not in case.reduced:
                        bad = (bits != clean[name]) & ~inside
                        if bool(bad.any()):
                            n, first, last = _where(bad)
                            raise NonFiniteError(f"{what}: containment: output '{name}' differs from the clean run in {n} elements outside the unit's region, "
                                                 f'first at (row {first[0]}, col {first[1]}), last at (row {last[0]}, col {last[1]})')
                    must = (unit.must if unit.must is not None else unit.affects).get(name)
                    if must is None or not op.data.dtype.is_floating_point or case.swallow is not None or name in case.reduced:
                        continue
                    limits = {_limit(case, n, kind) for n in group}
                    limit = 'nan' if kind == 'nan' else 'nonfinite' if 'nonfinite' in limits else 'any'
                    vals = bits.view(op.data.dtype).float()
                    if limit == 'nan':
                        bad = ~torch.isnan(vals)
                    elif limit == 'nonfinite':
                        bad = torch.isfinite(vals)
                    else:
                        continue
                    bad &= region_mask(must, op.rows, op.cols)
                    if bool(bad.any()):
                        n, first, last = _where(bad)
                        raise NonFiniteError(f"{what}: propagation: output '{name}' holds {n} {'non-NaN' if limit == 'nan' else 'finite'} values where the truth is "
                                             f"{'NaN' if limit == 'nan' else 'infinite or undefined'}, first at (row {first[0]}, col {first[1]}), "
                                             f'last at (row {last[0]}, col {last[1]})')
    return {'units': len(case.units), 'poisons': runs, 'swallows': int(case.swallow is not None)}


# ------------------------------------------------------------------ units of a packed batch

def seq_rows(lengths, i):
    s0 = sum(lengths[:i])
    return slice(s0, s0 + lengths[i])


def head_cols(d, h, blocks=1, stride=0):
    """Columns of head h (width d) in each of `blocks` column blocks `stride` apart."""
    return [b * stride + h * d + j for b in range(blocks) for j in range(d)]
