"""The GEMM operands of esme.lora.LoRA adapters in the packed forward, for either block.  A block has "up" projections
that share ONE LayerNorm-fed GEMM (attention: q, k, v; FFN: the up-projection -- SwiGLU: gate and fc) and one "down" projection behind a
producer kernel (attention: out; FFN: down).  Here: the refusals, the cache key, the derived entries, their expansion over a quantised base
and the per-call [x | u] buffers.  The blocks (esme/attention.py) keep which modules are wrapped, where each projection's rows sit in the
fused weight, where the base weight and its key come from, and the GEMM calls."""
from __future__ import annotations

from typing import NamedTuple

import torch

from esme import _hip
from esme.lora import INFERENCE_ONLY, LoRA, ext_width
from esme.nn import version_key


class ExtBlock(NamedTuple):
    """The extension columns [s B | 0] of a LoRA-extended weight on their own (`block`: (rows, X) bf16): what build() caches over a quantised
    base, where the base columns are expanded from the codes per call (expand).  (A tuple, so that Derived.tensors() finds the block.)"""
    block: torch.Tensor


def check_mode(training: bool, fast: bool = True) -> None:
    if training:
        raise NotImplementedError(INFERENCE_ONLY)
    if not fast:
        raise NotImplementedError("LoRA adapters run in precision 'fast' only ('high', 'half' and 'exact' have no adapter path)")


def check_precision(mode: str) -> None:
    if mode != 'fast':
        raise NotImplementedError(f"precision {mode!r} has no LoRA adapter path: adapters run in precision 'fast' only")


def check_base(padded: bool, quantised: bool, qlora: bool) -> None:
    if padded:
        raise NotImplementedError('LoRA adapters are not implemented for padded layouts (head dim 24 / a width that is not a multiple of 64)')
    if quantised and not qlora:
        raise NotImplementedError('LoRA adapters need unquantised bfloat16 base weights (quantization= is not supported with adapters, '
                                  'unless they were attached with add_lora(quantized_base=True))')


def cache_key(fold: bool, selection, projections, sels, base_key, ln):
    """Key of a block's 'lora' entry: (fold, selection, scalings, base key or 'quantised base', versioned tensors).  `base_key`: of the base
    form of the up weight, None on a quantised base -- no copy of the base is kept there, and the folded A' carries `ln`."""
    wrapped = [(m, s) for m, s in zip(projections, sels) if s is not None]
    scalings = tuple(float(m.scaling) for m, _ in wrapped)
    params = [t for m, s in wrapped for t in m.params(s)]
    if base_key is None:
        return bool(fold), selection, scalings, 'quantised base', version_key(*params, *((ln.weight, ln.bias) if fold else ()))
    return bool(fold), selection, scalings, base_key, version_key(projections[-1].weight, *params)


def entries(derived, names, projections, lora_names, fold: bool, ln, base, base_key, place, tags=None):
    """The 'lora' entry of a block's esme.nn.Derived for the adapters `lora_names` selects (LoRA.select: None / empty: all) -- build()'s
    result, built once per cache_key().  `projections`: the up ones in the order of their rows in the fused weight, then the down one.
    `fold`: for the LayerNorm-folded up GEMM, whose epilogue multiplies the accumulator by rstd: A carries gamma of `ln` (fold_down) and the
    kernel writes LN(x) A^T / rstd.  `base` / `base_key`: the up weight as that GEMM reads it and its key, None on a quantised base.
    `tags`: names under which the key lists the selection per projection (sorted), else in projection order."""
    sels = [m.select(lora_names) if isinstance(m, LoRA) else None for m in projections]
    selection = tuple(s for s in sels if s is not None) if tags is None else tuple(sorted((t, s) for t, s in zip(tags, sels) if s is not None))
    key = cache_key(fold, selection, projections, sels, base_key, ln)
    return derived.get('lora', key, build, names, projections, sels, ln if fold else None, base, place)


def fold_down(A: torch.Tensor, ln):
    """(A' = bf16(gamma * A), c1A = rowsum(A'), bA = A beta): the folded GEMM's epilogue multiplies by rstd, so the kernel writes LN(x) A^T / rstd."""
    Af = A.float()
    A = (Af * ln.weight.data.float().unsqueeze(0)).to(torch.bfloat16).contiguous()
    c1A = A.float().sum(dim=1).contiguous()
    bA = (Af @ ln.bias.data.float()).contiguous() if ln.bias is not None else torch.zeros_like(c1A)
    return A, c1A, bA


def join(base, ext: torch.Tensor):
    """[base | ext], or over a quantised base (`base` None) the extension columns alone."""
    return ExtBlock(ext.contiguous()) if base is None else torch.cat((base, ext), dim=1).contiguous()


def down_entry(mod: LoRA, sel: tuple, quantised: bool):
    """(X, A, [W | s B | 0]) of a single wrapped projection."""
    A, B = mod.stacked(sel)
    X = ext_width(A.shape[0])
    ext = torch.zeros(B.shape[0], X, dtype=torch.bfloat16, device=B.device)
    ext[:, :B.shape[1]] = B.to(torch.bfloat16)
    return X, A.contiguous(), join(None if quantised else mod.weight.data, ext)


def build(names, projections, sels, ln, base, place):
    """{names[0]: (X, A, c1A, bA, [W | s B | 0]) or None, names[1]: (X, A, [W_d | s B | 0]) or None} of the adapters `sels` (select()) of
    `projections` (the up ones in the order of their rows in the fused weight, then the down one).  The A of all selected adapters of the
    up projections are stacked to one (R, E) operand of esme_hip_lora_down; s B of each sits in its own projection's rows at its column
    offset, zero elsewhere; `place(per-projection (rows, X) blocks)` orders those rows like the fused weight's.  `ln`: the LayerNorm folded
    into the up GEMM, or None.  `base`: the up weight as that GEMM reads it; None on a quantised base (the last elements are ExtBlocks)."""
    *ups, down = projections
    res = dict.fromkeys(names)
    blocks = [(i, *m.stacked(s)) for i, (m, s) in enumerate(zip(ups, sels)) if s is not None]
    if blocks:
        A = torch.cat([a for _, a, _ in blocks], dim=0).contiguous()
        X = ext_width(A.shape[0])
        A, c1A, bA = fold_down(A, ln) if ln is not None else (A, None, None)
        parts = [torch.zeros(m.out_features, X, dtype=torch.bfloat16, device=A.device) for m in ups]
        o = 0
        for i, a, b in blocks:
            parts[i][:, o:o + a.shape[0]] = b.to(torch.bfloat16)
            o += a.shape[0]
        res[names[0]] = (X, A, c1A, bA, join(base, place(parts)))
    if sels[-1] is not None:
        res[names[1]] = down_entry(down, sels[-1], base is None)
    return res


def ext_widths(lw) -> tuple:
    """(X of the up GEMM, X of the down GEMM) of a build() result (0: that GEMM has no adapter)."""
    return tuple(e[0] if e else 0 for e in lw.values())


def expand(q4, entry, fold: bool = False):
    """[W | s B | 0] of a build() entry: the cached tensor, or, on a quantised base, `q4` (that GEMM's esme.quantization.Q4Matrix) expanded into
    a (rows, K + X) view of the shared weight scratch with the cached block copied behind it -- per call; the GEMM that reads it is next."""
    we = entry[-1]
    if not isinstance(we, ExtBlock):
        return we
    w = (q4.folded(entry[0]) if fold else q4.plain(entry[0]))[0]
    w[:, q4.cols:].copy_(we.block)
    return w


def folded_operand(x, entry, x_stats, ln, ctx):
    """[x | u] for the LayerNorm-folded up GEMM: u from esme_hip_lora_down_ln on the statistics `x_stats` of `ln`, written next to x in the model's
    stream buffer ctx.lora_x when x is its stream and it is wide enough, else into a buffer x moves to once (a caller outside the model)."""
    X, A, c1A, bA = entry[:4]
    T, E = x.shape
    xe = ctx.lora_x if ctx is not None else None
    if xe is None or xe.data_ptr() != x.data_ptr() or xe.stride(0) != x.stride(0) or xe.shape[1] < E + X:
        xe = torch.empty(T, E + X, dtype=torch.bfloat16, device=x.device)
        xe[:, :E].copy_(x)
    _hip.lora_down(xe[:, :E], A, xe[:, E:E + X], ln=(x_stats, E, ln.eps, c1A, bA))
    return xe[:, :E + X]


def ln_operand(x, entry, ln):
    """[LN(x) | u] in a fresh (T, E + X) buffer: the LayerNorm kernel, then esme_hip_lora_down (the unfolded form)."""
    X, A = entry[:2]
    T, E = x.shape
    he = torch.empty(T, E + X, dtype=torch.bfloat16, device=x.device)
    ln(x, out=he[:, :E])
    _hip.lora_down(he[:, :E], A, he[:, E:])
    return he


def tail_buffer(T: int, K: int, entry, device):
    """The operand of a down GEMM before its producer has run: (the (T, K + X) buffer, its first K columns for the producer to write)."""
    buf = torch.empty(T, K + entry[0], dtype=torch.bfloat16, device=device)
    return buf, buf[:, :K]


def fill_tail(buf, head, entry):
    """... and after: esme_hip_lora_down fills the columns behind what the producer wrote into `head`; returns the buffer."""
    _hip.lora_down(head, entry[1], buf[:, head.shape[1]:])
    return buf
