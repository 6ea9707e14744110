"""ctypes binding of include/esme_hip_segment_mean_bwd.h (csrc/segment_mean_bwd.hip): the backward of the per-sequence mean.

The entry point lives in a header of its own, so it has a signature table of its own; every call goes through
`_hip.load()`, the one handle of libesme_hip.so (a recorder installed over `_hip._lib` sees these calls too)."""
from __future__ import annotations

import ctypes
from ctypes import c_int, c_int64, c_void_p
from typing import Optional

import torch

from esme import _hip

ROWS = 32           # ESME_HIP_SEGMENT_MEAN_BWD_ROWS: rows of d_x per workgroup (no influence on the result)

SIGNATURES = {
    'esme_hip_segment_mean_bwd': (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int64, c_int, c_void_p, c_int64, c_int, c_void_p]),
}


def bind(lib) -> None:
    """Type the entry points on a ctypes handle of the library (idempotent; AttributeError if the library lacks one)."""
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args


def _lib():
    lib = _hip.load()
    if isinstance(lib, ctypes.CDLL):         # (a recorder wraps a handle that was typed before it was installed)
        bind(lib)
    return lib


def segment_mean_bwd(d_y: torch.Tensor, cu_lens: torch.Tensor, rows: int, d_x: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d_x (rows, E) of y = segment_mean(x, cu_lens) given d_y (B, E), bfloat16 or float32 (esme_hip_segment_mean_bwd): every row of a
    sequence gets d_y[s] / len_s (fp32 division, rounded once to d_y's dtype); rows before cu_lens[0] and from cu_lens[B] on are
    zeros.  cu_lens: int32 (B + 1) on the device; it is not read on the host.  d_y and `d_x` (if given: same dtype, (rows, E)): unit
    column stride, a row stride that is a multiple of 16 bytes.  Every element of `d_x` is written."""
    if d_y.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f'segment_mean_bwd: expected bfloat16 or float32, got {d_y.dtype}')
    yp, ldy = _hip._rows2d(d_y, 'segment_mean_bwd d_y', d_y.dtype)
    B, E = d_y.shape
    if cu_lens.dim() != 1 or cu_lens.numel() != B + 1:
        raise ValueError(f'segment_mean_bwd: cu_lens must be ({B + 1},) for d_y of {B} rows, got shape {tuple(cu_lens.shape)}')
    if d_x is None:
        d_x = torch.empty(int(rows), E, dtype=d_y.dtype, device=d_y.device)
    if d_x.dim() != 2 or d_x.shape != (int(rows), E):
        raise ValueError(f'segment_mean_bwd: d_x must be ({int(rows)}, {E}), got shape {tuple(d_x.shape)}')
    xp, ldx = _hip._rows2d(d_x, 'segment_mean_bwd d_x', d_y.dtype)
    with _hip._Traced('segment_mean_bwd', (int(rows), E, B)):
        _hip._check(_lib().esme_hip_segment_mean_bwd(yp, ldy, _hip._dev(cu_lens.contiguous(), 'segment_mean_bwd cu_lens', torch.int32), B, int(rows), E, xp, ldx,
                                                     1 if d_y.dtype == torch.float32 else 0, _hip._stream()), 'esme_hip_segment_mean_bwd')
    return d_x
