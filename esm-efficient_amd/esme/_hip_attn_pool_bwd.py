"""ctypes binding of include/esme_hip_attn_pool_bwd.h (csrc/pool_bwd.hip): the backward of the attention-pooling kernel.

The entry points live in a header of their own, so they have a signature table of their own; every call goes through
`_hip.load()`, the one handle of libesme_hip.so (a recorder installed over `_hip._lib` sees these calls too)."""
from __future__ import annotations

import ctypes
from ctypes import c_int, c_int64, c_void_p
from typing import Optional

import torch

from esme import _hip

SIGNATURES = {
    'esme_hip_attn_pool_bwd_workspace_bytes': (c_int64, [c_int, c_int64, c_int, c_int, c_int]),
    'esme_hip_attn_pool_bwd': (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_int64,
                                       c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
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


def workspace_bytes(B: int, T: int, E: int, heads: int, n_cls: int) -> int:
    n = _lib().esme_hip_attn_pool_bwd_workspace_bytes(int(B), int(T), int(E), int(heads), int(n_cls))
    if n < 0:
        _hip._check(n, 'esme_hip_attn_pool_bwd_workspace_bytes')
    return int(n)


def attn_pool_bwd(x: torch.Tensor, cu_lens: torch.Tensor, U: torch.Tensor, d_out: torch.Tensor, heads: int, n_cls: int,
                  need_dx: bool = True, dx: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """(dx or None, dU) of out = attn_pool(x, cu_lens, U) given d_out (esme_hip_attn_pool_bwd).  x (T, E) bfloat16 or float32 with
    contiguous rows, U (n_cls * heads, E) float32 contiguous (the forward's operands); d_out (B, n_cls, E) in x's dtype.  dx has x's
    dtype and is allocated as zeros (the kernel writes the rows of the sequences only); dU is float32.  need_dx=False skips the work
    that feeds only dx and returns None for it; dU is the same bits either way."""
    if x.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f'attn_pool_bwd: expected bfloat16 or float32 embeddings, got {x.dtype}')
    xp, ldx = _hip._rows2d(x, 'attn_pool_bwd x', x.dtype)
    if cu_lens.dtype != torch.int32:
        cu_lens = cu_lens.to(torch.int32)
    cu_lens = cu_lens.contiguous()
    T, E = x.shape
    B = cu_lens.numel() - 1
    J = int(n_cls) * int(heads)
    if U.dtype != torch.float32 or tuple(U.shape) != (J, E) or not U.is_contiguous():
        raise ValueError(f'attn_pool_bwd: U must be a contiguous float32 ({J}, {E}) tensor')
    if d_out.dtype != x.dtype or tuple(d_out.shape) != (B, n_cls, E):
        raise ValueError(f'attn_pool_bwd: d_out must be ({B}, {n_cls}, {E}) {x.dtype}, got {tuple(d_out.shape)} {d_out.dtype}')
    if d_out.stride(2) != 1 or d_out.stride(1) != E:
        d_out = d_out.contiguous()
    gp, ldg = _hip._dev(d_out, 'attn_pool_bwd d_out', x.dtype), (d_out.stride(0) if B > 1 else n_cls * E)
    dxp, lddx = None, 0
    if need_dx:
        if dx is None:
            dx = torch.zeros(T, E, dtype=x.dtype, device=x.device)
        if dx.dtype != x.dtype or tuple(dx.shape) != (T, E):
            raise ValueError(f'attn_pool_bwd: dx must be ({T}, {E}) {x.dtype}')
        dxp, lddx = _hip._rows2d(dx, 'attn_pool_bwd dx', x.dtype)
    else:
        dx = None
    dU = torch.empty(J, E, dtype=torch.float32, device=x.device)
    if workspace is None:
        workspace = torch.empty(workspace_bytes(B, T, E, heads, n_cls), dtype=torch.uint8, device=x.device)
    with _hip._Traced('attn_pool_bwd', (B, T, E, int(heads), int(n_cls), bool(need_dx))):
        _hip._check(_lib().esme_hip_attn_pool_bwd(xp, ldx, _hip._dev(cu_lens, 'cu_lens', torch.int32), B, T, E, int(heads), int(n_cls),
                                                  _hip._dev(U, 'attn_pool_bwd U', torch.float32), gp, ldg, dxp, lddx, dU.data_ptr(),
                                                  _hip._dev(workspace, 'attn_pool_bwd workspace', torch.uint8), workspace.numel(),
                                                  1 if x.dtype == torch.float32 else 0, _hip._stream()),
                    'esme_hip_attn_pool_bwd')
    return dx, dU
