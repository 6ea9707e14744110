"""ctypes binding of include/esme_hip_contacts.h (csrc/contacts.hip): contact logits reduced from the attention maps layer by layer.

The entry points live in a header of their own, so they have a signature table of their own; every call goes through
`_hip.load()`, the one handle of libesme_hip.so (a recorder installed over `_hip._lib` sees these calls too)."""
from __future__ import annotations

import ctypes
from ctypes import c_float, c_int, c_int64, c_void_p
from typing import Optional

import torch

from esme import _hip

SIGNATURES = {
    'esme_hip_contact_workspace_bytes': (c_int64, [c_int, c_int64, c_int]),
    'esme_hip_contact_layer': (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int64, c_int, c_int, c_int, c_float, c_int, c_int,
                                       c_int, c_void_p, c_float, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
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
    n = _lib().esme_hip_contact_workspace_bytes(int(B), int(T), int(H))
    if n < 0:
        _hip._check(n, 'esme_hip_contact_workspace_bytes')
    return int(n)


def map_offsets(cu_lens: torch.Tensor, trim_front: int, trim_back: int, blocks: int = 1):
    """(n (B) int64, map_off (B) int64, total) on cu_lens' device: sequence s owns `blocks` row-major n_s x n_s blocks at map_off[s]
    (block i at map_off[s] + i * n_s^2), n_s = its length without the trimmed rows; a sequence trimmed to nothing owns nothing."""
    lens = (cu_lens[1:] - cu_lens[:-1]).to(torch.int64)
    n = (lens - (trim_front + trim_back)).clamp_(min=0)
    sq = n * n * int(blocks)
    off = torch.cumsum(sq, 0) - sq
    return n, off, int(sq.sum())


def contact_layer(q: torch.Tensor, k: torch.Tensor, cu_lens: torch.Tensor, max_len: int, heads: int, head_dim: int, softmax_scale: float,
                  w: torch.Tensor, bias: float, init: bool, out: torch.Tensor, map_off: torch.Tensor, workspace: torch.Tensor,
                  q_prescaled: bool = False, trim_front: int = 1, trim_back: int = 1) -> None:
    """One layer's sum_h w[h] N^(h) into the packed fp32 map `out` (esme_hip_contact_layer).  q, k: (T, H * d) bfloat16 views with one
    row stride; w: float32 (H) on the device; map_off: int64 (B); workspace: uint8, at least workspace_bytes(B, T, H)."""
    qp, ld = _hip._rows2d(q, 'contact_layer q')
    kp, ldk = _hip._rows2d(k, 'contact_layer k')
    if ld != ldk or q.shape != k.shape or q.shape[1] != heads * head_dim:
        raise ValueError(f'contact_layer: q and k must be (T, {heads * head_dim}) views with one row stride, got {tuple(q.shape)} / {tuple(k.shape)}, '
                         f'strides {ld} / {ldk}')
    T, B = q.shape[0], cu_lens.numel() - 1
    if w.numel() != heads or not w.is_contiguous() or map_off.numel() != B or not map_off.is_contiguous() or not out.is_contiguous():
        raise ValueError('contact_layer: w must be a contiguous float32 (H) tensor, map_off a contiguous int64 (B) tensor, out contiguous')
    with _hip._Traced('contact_layer', (B, T, heads, head_dim)):
        _hip._check(_lib().esme_hip_contact_layer(qp, kp, ld, _hip._dev(cu_lens, 'cu_lens', torch.int32), B, T, int(heads), int(head_dim), int(max_len),
                                                  float(softmax_scale), int(bool(q_prescaled)), int(trim_front), int(trim_back),
                                                  _hip._dev(w, 'contact_layer w', torch.float32), float(bias), int(bool(init)),
                                                  _hip._dev(out, 'contact_layer map', torch.float32), _hip._dev(map_off, 'map_off', torch.int64),
                                                  _hip._dev(workspace, 'contact_layer workspace', torch.uint8), workspace.numel(), _hip._stream()),
                    'esme_hip_contact_layer')
