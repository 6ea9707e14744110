"""ctypes binding of include/esme_hip_contact_features.h (csrc/contacts.hip): the contact regression's features at chosen residue pairs.

A header of its own, so a signature table of its own; every call goes through `_hip.load()`, the one handle of libesme_hip.so (a
recorder installed over `_hip._lib` sees these calls too)."""
from __future__ import annotations

import ctypes
from ctypes import c_float, c_int, c_int64, c_void_p

import torch

from esme import _hip

SIGNATURES = {
    'esme_hip_contact_features_workspace_bytes': (c_int64, [c_int, c_int64, c_int]),
    'esme_hip_contact_features': (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int64, c_int, c_int, c_int, c_float, c_int, c_int,
                                          c_int, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p]),
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
    n = _lib().esme_hip_contact_features_workspace_bytes(int(B), int(T), int(H))
    if n < 0:
        _hip._check(n, 'esme_hip_contact_features_workspace_bytes')
    return int(n)


def contact_features(q: torch.Tensor, k: torch.Tensor, cu_lens: torch.Tensor, max_len: int, heads: int, head_dim: int, softmax_scale: float,
                     pairs: torch.Tensor, feat: torch.Tensor, col0: int, workspace: torch.Tensor, q_prescaled: bool = False,
                     trim_front: int = 1, trim_back: int = 1) -> None:
    """One layer's N^(h)_ij at the listed pairs into feat[:, col0 : col0 + H] (esme_hip_contact_features).  q, k: (T, H * d) bfloat16
    views with one row stride; pairs: contiguous int32 (P, 3) rows (s, i, j) on the device; feat: float32 (P, >= col0 + H) with unit
    column stride; workspace: uint8, at least workspace_bytes(B, T, H).  The pair list is not validated here (out-of-range rows come
    back as NaN)."""
    qp, ld = _hip._rows2d(q, 'contact_features q')
    kp, ldk = _hip._rows2d(k, 'contact_features k')
    if ld != ldk or q.shape != k.shape or q.shape[1] != heads * head_dim:
        raise ValueError(f'contact_features: q and k must be (T, {heads * head_dim}) views with one row stride, got {tuple(q.shape)} / {tuple(k.shape)}, '
                         f'strides {ld} / {ldk}')
    T, B = q.shape[0], cu_lens.numel() - 1
    if pairs.dim() != 2 or pairs.shape[1] != 3 or not pairs.is_contiguous():
        raise ValueError(f'contact_features: pairs must be a contiguous int32 (P, 3) tensor, got {tuple(pairs.shape)}')
    P = pairs.shape[0]
    if feat.dim() != 2 or feat.shape[0] != P or feat.shape[1] < col0 + heads or (P > 1 and feat.stride(0) < feat.shape[1]) or feat.stride(1) != 1:
        raise ValueError(f'contact_features: feat must be a float32 ({P}, >= {col0 + heads}) tensor with unit column stride, got {tuple(feat.shape)}')
    ld_feat = feat.stride(0) if P > 1 else max(feat.stride(0), feat.shape[1])
    with _hip._Traced('contact_features', (B, T, heads, head_dim, P)):
        _hip._check(_lib().esme_hip_contact_features(qp, kp, ld, _hip._dev(cu_lens, 'cu_lens', torch.int32), B, T, int(heads), int(head_dim), int(max_len),
                                                     float(softmax_scale), int(bool(q_prescaled)), int(trim_front), int(trim_back),
                                                     _hip._dev(pairs, 'contact_features pairs', torch.int32), P,
                                                     _hip._dev(feat, 'contact_features feat', torch.float32), ld_feat, int(col0),
                                                     _hip._dev(workspace, 'contact_features workspace', torch.uint8), workspace.numel(), _hip._stream()),
                    'esme_hip_contact_features')
