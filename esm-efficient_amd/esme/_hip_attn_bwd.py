"""ctypes binding of include/esme_hip_attn_bwd.h (csrc/attn_bwd.hip): the backward of the varlen attention kernel.

The entry points live in a header of their own, so they have a signature table of their own; every call goes through
`_hip.load()`, the one handle of libesme_hip.so (a recorder installed over `_hip._lib` sees these calls too)."""
from __future__ import annotations

import ctypes
from ctypes import c_float, c_int, c_int64, c_void_p
from typing import Optional

import torch

from esme import _hip

SUPPORTED_HEAD_DIMS = (32, 64)

SIGNATURES = {
    'esme_hip_attn_varlen_bwd_workspace_bytes': (c_int64, [c_int, c_int64, c_int]),
    'esme_hip_attn_varlen_bwd': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int, c_int64,
                                         c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
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


def workspace_bytes(B: int, T: int, H: int) -> int:
    n = _lib().esme_hip_attn_varlen_bwd_workspace_bytes(int(B), int(T), int(H))
    if n < 0:
        _hip._check(n, 'esme_hip_attn_varlen_bwd_workspace_bytes')
    return int(n)


def attn_varlen_bwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, o: torch.Tensor, d_o: torch.Tensor, cu_lens: torch.Tensor,
                    max_len: int, heads: int, softmax_scale: float, dq: Optional[torch.Tensor] = None, dk: Optional[torch.Tensor] = None,
                    dv: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """(dq, dk, dv) of out = attn_varlen(q, k, v) given d_o (esme_hip_attn_varlen_bwd).  q, k, v: (T, H * d) bfloat16 views with one row
    stride (the operands the forward consumed); o, d_o: (T, H * d) bfloat16, any row stride.  Without dq / dk / dv the three gradients
    are the column blocks of one new (T, 3 H d) buffer; rows that belong to no sequence are zero there."""
    qp, ld = _hip._rows2d(q, 'attn_varlen_bwd q')
    kp, ldk = _hip._rows2d(k, 'attn_varlen_bwd k')
    vp, ldv = _hip._rows2d(v, 'attn_varlen_bwd v')
    T, E = q.shape
    if not (ld == ldk == ldv) or k.shape != q.shape or v.shape != q.shape or o.shape != q.shape or d_o.shape != q.shape or E % heads:
        raise ValueError(f'attn_varlen_bwd: q, k, v must be (T, H * d) views with one row stride and o, d_o of the same shape, got '
                         f'{tuple(q.shape)} / {tuple(k.shape)} / {tuple(v.shape)} / {tuple(o.shape)} / {tuple(d_o.shape)}, strides {ld} / {ldk} / {ldv}')
    op, ldo = _hip._rows2d(o, 'attn_varlen_bwd o')
    gp, ldg = _hip._rows2d(d_o, 'attn_varlen_bwd d_o')
    if dq is None:
        buf = torch.zeros(T, 3 * E, dtype=torch.bfloat16, device=q.device)      # (the kernel writes the rows of the sequences only)
        dq, dk, dv = buf[:, :E], buf[:, E:2 * E], buf[:, 2 * E:]
    dqp, ldq = _hip._rows2d(dq, 'attn_varlen_bwd dq')
    dkp, ldk2 = _hip._rows2d(dk, 'attn_varlen_bwd dk')
    dvp, ldv2 = _hip._rows2d(dv, 'attn_varlen_bwd dv')
    if not (ldq == ldk2 == ldv2) or not (dq.shape == dk.shape == dv.shape == q.shape):
        raise ValueError('attn_varlen_bwd: dq, dk, dv must be (T, H * d) views with one shared row stride')
    B = cu_lens.numel() - 1
    if workspace is None:
        workspace = torch.empty(workspace_bytes(B, T, heads), dtype=torch.uint8, device=q.device)
    with _hip._Traced('attn_varlen_bwd', (B, T, heads, E // heads)):
        _hip._check(_lib().esme_hip_attn_varlen_bwd(qp, kp, vp, ld, op, ldo, gp, ldg, _hip._dev(cu_lens, 'cu_lens', torch.int32), B, T, int(heads),
                                                    E // heads, int(max_len), float(softmax_scale), dqp, dkp, dvp, ldq,
                                                    _hip._dev(workspace, 'attn_varlen_bwd workspace', torch.uint8), workspace.numel(), _hip._stream()),
                    'esme_hip_attn_varlen_bwd')
    return dq, dk, dv
