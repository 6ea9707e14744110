"""ctypes binding of include/esme_hip_attn_maps.h (csrc/attn_maps.hip): the attention maps of chosen heads of one layer, written out.

A header of its own, so a signature table of its own; every call goes through `_hip.load()`, the one handle of libesme_hip.so (a
recorder installed over `_hip._lib` sees these calls too)."""
from __future__ import annotations

import ctypes
from ctypes import c_float, c_int, c_int64, c_void_p
from typing import Optional

import torch

from esme import _hip, _hip_contacts

SIGNATURES = {
    'esme_hip_attn_maps_workspace_bytes': (c_int64, [c_int, c_int64, c_int]),
    'esme_hip_attn_maps': (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int64, c_int, c_int, c_int, c_float, c_int, c_void_p, c_int,
                                   c_void_p, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
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


def workspace_bytes(B: int, T: int, n_heads: int) -> int:
    n = _lib().esme_hip_attn_maps_workspace_bytes(int(B), int(T), int(n_heads))
    if n < 0:
        _hip._check(n, 'esme_hip_attn_maps_workspace_bytes')
    return int(n)


def map_offsets(cu_lens: torch.Tensor, blocks: int = 1):
    """(S (B) int64, map_off (B) int64, total) on cu_lens' device: sequence s owns `blocks` row-major S_s x S_s blocks, blocks * S_s^2
    elements at map_off[s] (block i at map_off[s] + i * S_s^2); an empty sequence owns nothing."""
    return _hip_contacts.map_offsets(cu_lens, 0, 0, blocks)


def attn_maps(q: torch.Tensor, k: torch.Tensor, cu_lens: torch.Tensor, max_len: int, heads: int, head_dim: int, softmax_scale: float,
              head_list: torch.Tensor, out: torch.Tensor, map_off: torch.Tensor, slot0: int, workspace: torch.Tensor,
              head_weights: Optional[torch.Tensor] = None, q_prescaled: bool = False) -> None:
    """softmax(q k^T * scale) of the heads in `head_list` into `out` (esme_hip_attn_maps).  q, k: (T, H * d) bfloat16 views with one row
    stride; head_list: contiguous int32 (n) on the device, each in [0, H) (the caller checks that: the library does not);
    out: contiguous float32 or bfloat16; map_off: int64 (B), in elements.  Without head_weights, head head_list[j] of sequence s goes to
    the S_s x S_s block at out + map_off[s] + (slot0 + j) * S_s^2; with head_weights (float32 (n) on the device) the one block at slot0
    holds sum_j head_weights[j] * P_j.  workspace: uint8, at least workspace_bytes(B, T, n)."""
    qp, ld = _hip._rows2d(q, 'attn_maps q')
    kp, ldk = _hip._rows2d(k, 'attn_maps k')
    if ld != ldk or q.shape != k.shape or q.shape[1] != heads * head_dim:
        raise ValueError(f'attn_maps: q and k must be (T, {heads * head_dim}) views with one row stride, got {tuple(q.shape)} / {tuple(k.shape)}, '
                         f'strides {ld} / {ldk}')
    T, B = q.shape[0], cu_lens.numel() - 1
    n = head_list.numel()
    if head_list.dim() != 1 or not head_list.is_contiguous() or map_off.numel() != B or not map_off.is_contiguous() or not out.is_contiguous():
        raise ValueError('attn_maps: head_list must be a contiguous int32 (n) tensor, map_off a contiguous int64 (B) tensor, out contiguous')
    if out.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f'attn_maps: out must be float32 or bfloat16, got {out.dtype}')
    if head_weights is not None and (head_weights.numel() != n or not head_weights.is_contiguous()):
        raise ValueError(f'attn_maps: head_weights must be a contiguous float32 ({n}) tensor')
    wp = None if head_weights is None else _hip._dev(head_weights, 'attn_maps head_weights', torch.float32)
    with _hip._Traced('attn_maps', (B, T, heads, head_dim, n)):
        _hip._check(_lib().esme_hip_attn_maps(qp, kp, ld, _hip._dev(cu_lens, 'cu_lens', torch.int32), B, T, int(heads), int(head_dim), int(max_len),
                                              float(softmax_scale), int(bool(q_prescaled)), _hip._dev(head_list, 'attn_maps head_list', torch.int32), n,
                                              wp, _hip._dev(out, 'attn_maps map'), int(out.dtype == torch.bfloat16),
                                              _hip._dev(map_off, 'map_off', torch.int64), int(slot0),
                                              _hip._dev(workspace, 'attn_maps workspace', torch.uint8), workspace.numel(), _hip._stream()),
                    'esme_hip_attn_maps')
