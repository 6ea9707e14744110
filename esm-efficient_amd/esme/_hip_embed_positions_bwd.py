"""ctypes binding of include/esme_hip_embed_positions_bwd.h (csrc/embed_positions_bwd.hip): the gradient of the learned-position table
of ESM-1b / ESM-1v.

The entry point lives in a header of its own, so it has a signature table of its own; every call goes through `_hip.load()`, the one
handle of libesme_hip.so (a recorder installed over `_hip._lib` sees these calls too)."""
from __future__ import annotations

import ctypes
from ctypes import c_int, c_int64, c_void_p
from typing import Optional

import torch

from esme import _hip

SIGNATURES = {
    'esme_hip_embed_positions_bwd': (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
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


def embed_positions_bwd(d_x: torch.Tensor, cu_lens: torch.Tensor, P: int, pos_offset: int, max_len: int,
                        d_pos: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d_pos (P, E) bfloat16 of the position half of x = embed_positions(...) on packed rows, given d_x (T, E) bfloat16
    (esme_hip_embed_positions_bwd): table row p + pos_offset gets the sum of row p of every sequence of `cu_lens` (int32 (B + 1,)) longer
    than p, p < max_len, in fp32 and ascending sequence order, rounded once; every other row is zeros.  d_x: unit column stride, a row
    stride that is a multiple of 8.  Every element of `d_pos` is written."""
    gp, ld = _hip._rows2d(d_x, 'embed_positions_bwd d_x')
    T, E = d_x.shape
    if cu_lens.dim() != 1 or cu_lens.numel() < 1 or not cu_lens.is_contiguous():
        raise ValueError(f'embed_positions_bwd: cu_lens must be a contiguous (B + 1,) tensor, got shape {tuple(cu_lens.shape)} stride {cu_lens.stride()}')
    if d_pos is None:
        d_pos = torch.empty(int(P), E, dtype=torch.bfloat16, device=d_x.device)
    if d_pos.shape != (int(P), E) or not d_pos.is_contiguous():
        raise ValueError(f'embed_positions_bwd: d_pos must be a contiguous ({P}, {E}) tensor, got shape {tuple(d_pos.shape)} stride {d_pos.stride()}')
    B = cu_lens.numel() - 1
    with _hip._Traced('embed_positions_bwd', (T, E, B, int(P))):
        _hip._check(_lib().esme_hip_embed_positions_bwd(gp, ld, _hip._dev(cu_lens, 'embed_positions_bwd cu_lens', torch.int32), B, T, E, int(P),
                                                        int(pos_offset), int(max_len),
                                                        _hip._dev(d_pos, 'embed_positions_bwd d_pos', torch.bfloat16), _hip._stream()),
                    'esme_hip_embed_positions_bwd')
    return d_pos
