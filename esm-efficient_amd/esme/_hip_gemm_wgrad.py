"""ctypes binding of include/esme_hip_gemm_wgrad.h (csrc/gemm_wgrad.hip): the weight gradient dW = dY^T X (and db) of a projection.

The entry points live in a header of their own, so they have a signature table of their own; every call goes through
`_hip.load()`, the one handle of libesme_hip.so (a recorder installed over `_hip._lib` sees these calls too)."""
from __future__ import annotations

import ctypes
from ctypes import c_int, c_int64, c_void_p
from typing import Optional

import torch

from esme import _hip

SIGNATURES = {
    'esme_hip_gemm_wgrad_workspace_bytes': (c_int64, [c_int64, c_int, c_int]),
    'esme_hip_gemm_wgrad': (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_int, c_void_p, c_int64, c_void_p, c_int,
                                    c_void_p, c_int64, c_void_p]),
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


def workspace_bytes(M: int, N: int, K: int) -> int:
    n = _lib().esme_hip_gemm_wgrad_workspace_bytes(int(M), int(N), int(K))
    if n < 0:
        _hip._check(n, 'esme_hip_gemm_wgrad_workspace_bytes')
    return int(n)


def gemm_wgrad(dy: torch.Tensor, x: torch.Tensor, bias: bool = False, out_dtype=torch.bfloat16, dw: Optional[torch.Tensor] = None,
               db: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """(dW (N, K), db (N) or None) of y = x W^T + b given dy (esme_hip_gemm_wgrad): dW = dy^T x, db = the column sums of dy.
    dy (M, N) and x (M, K) bfloat16 with contiguous rows (any row stride that is a multiple of 8); N and K multiples of 64.
    out_dtype bfloat16 or float32, the dtype of both results; `bias` asks for db.  The results are bit-equal from run to run and
    from device to device (no atomics; the row partition depends on the shape alone)."""
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f'gemm_wgrad: out_dtype must be bfloat16 or float32, got {out_dtype}')
    yp, ld_dy = _hip._rows2d(dy, 'gemm_wgrad dy')
    xp, ld_x = _hip._rows2d(x, 'gemm_wgrad x')
    M, N = dy.shape
    K = x.shape[1]
    if x.shape[0] != M:
        raise ValueError(f'gemm_wgrad: dy has {M} rows, x {x.shape[0]}')
    if dw is None:
        dw = torch.empty(N, K, dtype=out_dtype, device=dy.device)
    if dw.dtype != out_dtype or tuple(dw.shape) != (N, K):
        raise ValueError(f'gemm_wgrad: dw must be ({N}, {K}) {out_dtype}')
    wp, ld_dw = _hip._rows2d(dw, 'gemm_wgrad dw', out_dtype)
    bp = None
    if bias or db is not None:
        if db is None:
            db = torch.empty(N, dtype=out_dtype, device=dy.device)
        if db.dtype != out_dtype or tuple(db.shape) != (N,) or not db.is_contiguous():
            raise ValueError(f'gemm_wgrad: db must be a contiguous ({N},) {out_dtype} tensor')
        bp = _hip._dev(db, 'gemm_wgrad db', out_dtype)
    need = workspace_bytes(M, N, K)
    if workspace is None and need:
        workspace = torch.empty(need, dtype=torch.uint8, device=dy.device)
    sp, nb = (None, 0) if workspace is None else (_hip._dev(workspace, 'gemm_wgrad workspace', torch.uint8), workspace.numel())
    if M == 0:
        ld_dy, ld_x = max(ld_dy, N), max(ld_x, K)               # (an empty tensor's stride says nothing)
    with _hip._Traced('gemm_wgrad', (M, N, K, out_dtype == torch.float32, bp is not None)):
        _hip._check(_lib().esme_hip_gemm_wgrad(yp, ld_dy, xp, ld_x, M, N, K, wp, ld_dw, bp, 1 if out_dtype == torch.float32 else 0,
                                               sp, nb, _hip._stream()), 'esme_hip_gemm_wgrad')
    return dw, db
