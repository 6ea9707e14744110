"""ctypes binding of include/esme_hip_crf.h (csrc/crf.hip): a linear-chain CRF over packed sequences -- log Z by the forward
algorithm, its gradients by the backward algorithm, and Viterbi decoding.

The entry points live in a header of their own, so they have a signature table of their own; every call goes through
`_hip.load()`, the one handle of libesme_hip.so (a recorder installed over `_hip._lib` sees these calls too)."""
from __future__ import annotations

import ctypes
from ctypes import c_int, c_int64, c_void_p
from typing import Optional, Tuple

import torch

from esme import _hip

FREE = -1           # ESME_HIP_CRF_FREE: a chain row with every label allowed
SKIP = -2           # ESME_HIP_CRF_SKIP: a row outside the chain
MAX_C = 64          # ESME_HIP_CRF_MAX_C
PARTS = 1024        # ESME_HIP_CRF_PARTS: the sums over sequences run over min(B, PARTS) parts

_OPERANDS = [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int]
SIGNATURES = {
    'esme_hip_crf_bwd_workspace_bytes': (c_int64, [c_int64, c_int64, c_int]),
    'esme_hip_crf_decode_workspace_bytes': (c_int64, [c_int64, c_int]),
    'esme_hip_crf_fwd': (c_int, _OPERANDS + [c_void_p, c_void_p, c_void_p]),
    'esme_hip_crf_bwd': (c_int, _OPERANDS + [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_int64, c_void_p]),
    'esme_hip_crf_decode': (c_int, _OPERANDS + [c_void_p, c_int, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
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


def bwd_workspace_bytes(B: int, T: int, C: int) -> int:
    n = _lib().esme_hip_crf_bwd_workspace_bytes(int(B), int(T), int(C))
    if n < 0:
        _hip._check(n, 'esme_hip_crf_bwd_workspace_bytes')
    return int(n)


def decode_workspace_bytes(T: int, C: int) -> int:
    n = _lib().esme_hip_crf_decode_workspace_bytes(int(T), int(C))
    if n < 0:
        _hip._check(n, 'esme_hip_crf_decode_workspace_bytes')
    return int(n)


def _vec(t, n, what, dtype):
    if t.dim() != 1 or t.numel() != n or not t.is_contiguous():
        raise ValueError(f'{what} must be a contiguous ({n},) tensor, got shape {tuple(t.shape)} stride {t.stride()}')
    return _hip._dev(t, what, dtype)


def _operands(emissions, transitions, start, end, cu_lens, tags, what):
    ep, lde = _hip._rows2d(emissions, f'{what} emissions', torch.float32)
    T, C = emissions.shape
    if transitions.shape != (C, C) or not transitions.is_contiguous():
        raise ValueError(f'{what}: transitions must be a contiguous ({C}, {C}) tensor, got shape {tuple(transitions.shape)}')
    if cu_lens.dim() != 1 or cu_lens.numel() < 1:
        raise ValueError(f'{what}: cu_lens must be a (B + 1,) tensor, got shape {tuple(cu_lens.shape)}')
    B = cu_lens.numel() - 1
    return (ep, lde, _hip._dev(transitions, f'{what} transitions', torch.float32), _vec(start, C, f'{what} start', torch.float32),
            _vec(end, C, f'{what} end', torch.float32), _vec(cu_lens, B + 1, f'{what} cu_lens', torch.int32),
            _vec(tags, T, f'{what} tags', torch.int32), B, T, C)


def crf_fwd(emissions: torch.Tensor, transitions: torch.Tensor, start: torch.Tensor, end: torch.Tensor, cu_lens: torch.Tensor,
            tags: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(logz (B,), alpha (T, C)) float32 of esme_hip_crf_fwd: the log-partition function of every sequence's chain under the
    constraints of `tags` (int32 (T,): a label, FREE or SKIP per row) and the forward variables the backward reads.  emissions (T, C)
    float32 with unit column stride; transitions (C, C), start, end (C,) float32; cu_lens (B + 1,) int32."""
    ops = _operands(emissions, transitions, start, end, cu_lens, tags, 'crf_fwd')
    B, T, C = ops[-3:]
    logz = torch.empty(B, dtype=torch.float32, device=emissions.device)
    alpha = (torch.empty if B else torch.zeros)(T, C, dtype=torch.float32, device=emissions.device)      # (no sequence: the library writes nothing)
    with _hip._Traced('crf_fwd', (B, T, C)):
        _hip._check(_lib().esme_hip_crf_fwd(*ops, logz.data_ptr(), alpha.data_ptr(), _hip._stream()), 'esme_hip_crf_fwd')
    return logz, alpha


def crf_bwd(emissions: torch.Tensor, transitions: torch.Tensor, start: torch.Tensor, end: torch.Tensor, cu_lens: torch.Tensor,
            tags: torch.Tensor, alpha: torch.Tensor, logz: torch.Tensor, grad: torch.Tensor, want_params: bool = True,
            workspace: Optional[torch.Tensor] = None):
    """(d_emissions (T, C), d_transitions (C, C), d_start (C,), d_end (C,)) float32 of sum_b grad[b] logz[b] (esme_hip_crf_bwd);
    `alpha`, `logz` as the forward returned them, `grad` (B,) float32 on the device.  The last three are None without `want_params`.
    With grad = 1 the rows of d_emissions are the posterior marginals."""
    ops = _operands(emissions, transitions, start, end, cu_lens, tags, 'crf_bwd')
    B, T, C = ops[-3:]
    dev = emissions.device
    d_e = (torch.empty if B else torch.zeros)(T, C, dtype=torch.float32, device=dev)      # (no sequence: the library writes no row)
    d_t = d_s = d_n = None
    if want_params:
        d_t = torch.empty(C, C, dtype=torch.float32, device=dev)
        d_s = torch.empty(C, dtype=torch.float32, device=dev)
        d_n = torch.empty(C, dtype=torch.float32, device=dev)
        if workspace is None:
            workspace = torch.empty(bwd_workspace_bytes(B, T, C), dtype=torch.uint8, device=dev)
    p = lambda t: None if t is None else t.data_ptr()
    if alpha.shape != (T, C) or not alpha.is_contiguous():
        raise ValueError(f'crf_bwd: alpha must be a contiguous ({T}, {C}) tensor, got shape {tuple(alpha.shape)}')
    with _hip._Traced('crf_bwd', (B, T, C)):
        _hip._check(_lib().esme_hip_crf_bwd(*ops, _hip._dev(alpha, 'crf_bwd alpha', torch.float32), _vec(logz, B, 'crf_bwd logz', torch.float32),
                                            _vec(grad, B, 'crf_bwd grad', torch.float32), d_e.data_ptr(), C, int(bool(want_params)),
                                            p(d_t), p(d_s), p(d_n), p(workspace), 0 if workspace is None else workspace.numel(),
                                            _hip._stream()), 'esme_hip_crf_bwd')
    return d_e, d_t, d_s, d_n


def crf_decode(emissions: torch.Tensor, transitions: torch.Tensor, start: torch.Tensor, end: torch.Tensor, cu_lens: torch.Tensor,
               tags: torch.Tensor, fill: int = -100, dtype=torch.int64, workspace: Optional[torch.Tensor] = None):
    """(path (T,) `dtype` int64 / int32, score (B,) float32) of esme_hip_crf_decode: the best label path of every chain under the
    constraints of `tags` (ties: the lowest predecessor, the lowest final label), `fill` on the rows outside chains."""
    if dtype not in (torch.int32, torch.int64):
        raise TypeError(f'crf_decode: path dtype must be int32 or int64, got {dtype}')
    ops = _operands(emissions, transitions, start, end, cu_lens, tags, 'crf_decode')
    B, T, C = ops[-3:]
    dev = emissions.device
    path = torch.empty(T, dtype=dtype, device=dev) if B else torch.full((T,), int(fill), dtype=dtype, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    if workspace is None:
        workspace = torch.empty(decode_workspace_bytes(T, C), dtype=torch.uint8, device=dev)
    with _hip._Traced('crf_decode', (B, T, C)):
        _hip._check(_lib().esme_hip_crf_decode(*ops, path.data_ptr(), int(dtype == torch.int64), int(fill), score.data_ptr(),
                                               _hip._dev(workspace, 'crf_decode workspace', torch.uint8), workspace.numel(), _hip._stream()),
                    'esme_hip_crf_decode')
    return path, score
