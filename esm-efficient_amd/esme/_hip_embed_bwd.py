"""ctypes binding of include/esme_hip_embed_bwd.h (csrc/embed_bwd.hip): the gradient of the token-embedding table.

The entry points live in a header of their own, so they have a signature table of their own; every call goes through
`_hip.load()`, the one handle of libesme_hip.so (a recorder installed over `_hip._lib` sees these calls too)."""
from __future__ import annotations

import ctypes
from ctypes import c_int, c_int64, c_void_p
from typing import Optional

import torch

from esme import _hip

ROWS = 256          # ESME_HIP_EMBED_BWD_ROWS: rows per chunk of the first launch (part of the summation order)
MAX_V = 64          # ESME_HIP_EMBED_BWD_MAX_V

SIGNATURES = {
    'esme_hip_embed_bwd_workspace_bytes': (c_int64, [c_int64, c_int, c_int]),
    'esme_hip_embed_bwd': (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p]),
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


def workspace_bytes(T: int, E: int, V: int) -> int:
    n = _lib().esme_hip_embed_bwd_workspace_bytes(int(T), int(E), int(V))
    if n < 0:
        _hip._check(n, 'esme_hip_embed_bwd_workspace_bytes')
    return int(n)


def embed_bwd(d_x: torch.Tensor, tokens: torch.Tensor, V: int, mask_idx: int = -1, pad_idx: int = -1,
              d_table: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d_table (V, E) bfloat16 of x = embed(tokens, table, mask_idx, pad_idx) given d_x (T, E) bfloat16 (esme_hip_embed_bwd): per id the
    sum of its rows of d_x, in fp32 and a fixed order, rounded once; rows of ids that do not occur, of `mask_idx` and of `pad_idx` are
    zeros.  d_x: unit column stride, a row stride that is a multiple of 8; tokens: int64 (T,).  Every element of `d_table` is written."""
    gp, ld = _hip._rows2d(d_x, 'embed_bwd d_x')
    T, E = d_x.shape
    if tokens.dim() != 1 or tokens.numel() != T or not tokens.is_contiguous():
        raise ValueError(f'embed_bwd: tokens must be a contiguous ({T},) tensor, got shape {tuple(tokens.shape)} stride {tokens.stride()}')
    if d_table is None:
        d_table = torch.empty(V, E, dtype=torch.bfloat16, device=d_x.device)
    if d_table.shape != (V, E) or not d_table.is_contiguous():
        raise ValueError(f'embed_bwd: d_table must be a contiguous ({V}, {E}) tensor, got shape {tuple(d_table.shape)} stride {d_table.stride()}')
    if workspace is None:
        workspace = torch.empty(workspace_bytes(T, E, V), dtype=torch.uint8, device=d_x.device)
    with _hip._Traced('embed_bwd', (T, E, V)):
        _hip._check(_lib().esme_hip_embed_bwd(gp, ld, _hip._dev(tokens, 'embed_bwd tokens', torch.int64), T, E, int(V), int(mask_idx), int(pad_idx),
                                              _hip._dev(d_table, 'embed_bwd d_table', torch.bfloat16),
                                              _hip._dev(workspace, 'embed_bwd workspace', torch.uint8), workspace.numel(), _hip._stream()),
                    'esme_hip_embed_bwd')
    return d_table
