"""ctypes binding of include/esme_hip_linear_xent.h (csrc/linear_xent.hip): a linear layer fused with the cross-entropy of its logits.

The entry points live in a header of their own, so they have a signature table of their own; every call goes through
`_hip.load()`, the one handle of libesme_hip.so (a recorder installed over `_hip._lib` sees these calls too)."""
from __future__ import annotations

import ctypes
from ctypes import c_int, c_int64, c_void_p
from typing import Optional, Tuple

import torch

from esme import _hip

TILE = 64           # ESME_HIP_LINEAR_XENT_TILE: rows per workgroup, the unit of the L / D / db partials
CHUNK = 512         # ESME_HIP_LINEAR_XENT_CHUNK: rows per chunk of the dW contraction
MAX_C = 64          # ESME_HIP_LINEAR_XENT_MAX_C

_OPERANDS = [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int64, c_void_p, c_int64, c_int, c_int, c_int]
SIGNATURES = {
    'esme_hip_linear_xent_fwd_workspace_bytes': (c_int64, [c_int64]),
    'esme_hip_linear_xent_bwd_workspace_bytes': (c_int64, [c_int64, c_int, c_int]),
    'esme_hip_linear_xent_fwd': (c_int, _OPERANDS + [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    'esme_hip_linear_xent_bwd': (c_int, _OPERANDS + [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int,
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


def fwd_workspace_bytes(T: int) -> int:
    n = _lib().esme_hip_linear_xent_fwd_workspace_bytes(int(T))
    if n < 0:
        _hip._check(n, 'esme_hip_linear_xent_fwd_workspace_bytes')
    return int(n)


def bwd_workspace_bytes(T: int, E: int, C: int) -> int:
    n = _lib().esme_hip_linear_xent_bwd_workspace_bytes(int(T), int(E), int(C))
    if n < 0:
        _hip._check(n, 'esme_hip_linear_xent_bwd_workspace_bytes')
    return int(n)


def _operands(x, w, bias, labels, ignore_index, class_weight, mean, what):
    xp, ldx = _hip._rows2d(x, f'{what} x')
    wp, ldw = _hip._rows2d(w, f'{what} w')
    T, E = x.shape
    C = w.shape[0]
    if w.shape[1] != E:
        raise ValueError(f'{what}: w is {tuple(w.shape)} but x has {E} columns')
    if labels.dtype not in (torch.int32, torch.int64):
        raise TypeError(f'{what}: labels must be int32 or int64, got {labels.dtype}')
    if labels.dim() != 1 or labels.numel() != T or not labels.is_contiguous():
        raise ValueError(f'{what}: labels must be a contiguous ({T},) tensor, got shape {tuple(labels.shape)} stride {labels.stride()}')
    if bias is not None and (bias.shape != (C,) or not bias.is_contiguous()):
        raise ValueError(f'{what}: bias must be a contiguous ({C},) tensor, got shape {tuple(bias.shape)}')
    if class_weight is not None and (class_weight.shape != (C,) or not class_weight.is_contiguous()):
        raise ValueError(f'{what}: class_weight must be a contiguous ({C},) tensor, got shape {tuple(class_weight.shape)}')
    return (xp, ldx, wp, ldw, None if bias is None else _hip._dev(bias, f'{what} bias', torch.bfloat16),
            _hip._dev(labels, f'{what} labels'), int(labels.dtype == torch.int64), int(ignore_index),
            None if class_weight is None else _hip._dev(class_weight, f'{what} class_weight', torch.float32), T, E, C, int(bool(mean)))


def linear_xent_fwd(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], labels: torch.Tensor, ignore_index: int = -100,
                    class_weight: Optional[torch.Tensor] = None, mean: bool = True,
                    workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(sums, loss_rows, lse) of the cross-entropy of the logits x w^T + bias against `labels` (esme_hip_linear_xent_fwd), all float32:
    sums (4,) = [L, D, loss, 0] with L the sum of the rows' losses, D the sum of the kept rows' class weights and loss = L (`mean`
    False) or L / D (0 when D == 0); loss_rows (T,), lse (T,).  A row whose label is `ignore_index` or outside [0, C) is ignored.
    x (T, E), w (C, E) bfloat16 with unit column stride and row strides that are multiples of 8; labels int32 / int64 (T,)."""
    ops = _operands(x, w, bias, labels, ignore_index, class_weight, mean, 'linear_xent_fwd')
    T = x.shape[0]
    sums = torch.empty(4, dtype=torch.float32, device=x.device)
    loss_rows = torch.empty(T, dtype=torch.float32, device=x.device)
    lse = torch.empty(T, dtype=torch.float32, device=x.device)
    if workspace is None:
        workspace = torch.empty(fwd_workspace_bytes(T), dtype=torch.uint8, device=x.device)
    with _hip._Traced('linear_xent_fwd', (T, x.shape[1], w.shape[0])):
        _hip._check(_lib().esme_hip_linear_xent_fwd(*ops, loss_rows.data_ptr(), lse.data_ptr(), sums.data_ptr(),
                                                    _hip._dev(workspace, 'linear_xent_fwd workspace', torch.uint8), workspace.numel(),
                                                    _hip._stream()), 'esme_hip_linear_xent_fwd')
    return sums, loss_rows, lse


def linear_xent_bwd(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], labels: torch.Tensor, lse: torch.Tensor,
                    sums: torch.Tensor, grad: torch.Tensor, ignore_index: int = -100, class_weight: Optional[torch.Tensor] = None,
                    mean: bool = True, want_dx: bool = True, want_dw: bool = True, out_f32: bool = False,
                    d_x: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """(d_x, d_w, d_b) of the loss of `linear_xent_fwd` on the same operands (esme_hip_linear_xent_bwd); `lse`, `sums` as the forward
    returned them, `grad` the upstream gradient as a float32 device tensor of one element.  d_x (T, E) bfloat16 (None without
    `want_dx`; `d_x` may be given, e.g. a column block of a wider buffer); d_w (C, E) and d_b (C,) (None without a bias) in bfloat16 or
    (`out_f32`) float32, None without `want_dw`."""
    ops = _operands(x, w, bias, labels, ignore_index, class_weight, mean, 'linear_xent_bwd')
    T, E = x.shape
    C = w.shape[0]
    dev = x.device
    if grad.numel() != 1:
        raise ValueError(f'linear_xent_bwd: grad must hold one element, got shape {tuple(grad.shape)}')
    dxp, lddx = None, 0
    if want_dx:
        if d_x is None:
            d_x = torch.empty(T, E, dtype=torch.bfloat16, device=dev)
        if d_x.shape != (T, E):
            raise ValueError(f'linear_xent_bwd: d_x must be ({T}, {E}), got {tuple(d_x.shape)}')
        dxp, lddx = _hip._rows2d(d_x, 'linear_xent_bwd d_x')
    else:
        d_x = None
    d_w = d_b = None
    if want_dw:
        odt = torch.float32 if out_f32 else torch.bfloat16
        d_w = torch.empty(C, E, dtype=odt, device=dev)
        d_b = torch.empty(C, dtype=odt, device=dev) if bias is not None else None
    if workspace is None:
        workspace = torch.empty(bwd_workspace_bytes(T, E, C), dtype=torch.uint8, device=dev)
    with _hip._Traced('linear_xent_bwd', (T, E, C)):
        _hip._check(_lib().esme_hip_linear_xent_bwd(*ops, _hip._dev(lse, 'linear_xent_bwd lse', torch.float32),
                                                    _hip._dev(sums, 'linear_xent_bwd sums', torch.float32),
                                                    _hip._dev(grad, 'linear_xent_bwd grad', torch.float32),
                                                    int(bool(want_dx)), dxp, lddx, int(bool(want_dw)),
                                                    None if d_w is None else d_w.data_ptr(), None if d_b is None else d_b.data_ptr(),
                                                    int(bool(out_f32)), _hip._dev(workspace, 'linear_xent_bwd workspace', torch.uint8),
                                                    workspace.numel(), _hip._stream()), 'esme_hip_linear_xent_bwd')
    return d_x, d_w, d_b
