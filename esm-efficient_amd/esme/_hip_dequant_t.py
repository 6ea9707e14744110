"""ctypes binding of include/esme_hip_dequant_t.h (csrc/quant_t.hip): the transposing expansion of quantised weights, W^T (K, N) bf16
straight from the codes of W (N, K) -- the operand of dX = dY W when adapters are trained over a quantised base (esme.autograd.QuantFrozenLinear).

The entry points live in a header of their own, so they have a signature table of their own; every call goes through
`_hip.load()`, the one handle of libesme_hip.so (a recorder installed over `_hip._lib` sees these calls too)."""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_float, c_int, c_int64, c_void_p
from typing import Optional

import torch

from esme import _hip

SIGNATURES = {
    'esme_hip_dequantize_4bit_t': (c_int, [c_void_p, c_void_p, c_int64, c_int, POINTER(c_float), c_void_p, c_int64, c_void_p]),
    'esme_hip_dequantize_8bit_t': (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p]),
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


def _out(out: Optional[torch.Tensor], K: int, N: int, device, what: str):
    if out is None:                              # (the kernel stores 16 bytes at a time: a row stride that is a multiple of 8)
        out = torch.empty(K, (N + 7) // 8 * 8, dtype=torch.bfloat16, device=device)[:, :N]
    elif tuple(out.shape) != (K, N):
        raise ValueError(f'{what}: out shape {tuple(out.shape)} != {(K, N)}')
    op, ldo = _hip._rows2d(out, f'{what} out')
    return out, op, ldo


def dequantize_4bit_t(codes: torch.Tensor, absmax: torch.Tensor, codebook, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(K, N) bf16: out[k, n] = the value _hip.dequantize_4bit(codes, absmax, codebook) holds at [n, k], bit for bit; `out` may be a
    row-strided view (a scratch view, a column block of a wider buffer)."""
    _hip._dev(codes, 'dequantize_4bit_t codes', torch.uint8)
    _hip._dev(absmax, 'dequantize_4bit_t absmax', torch.float32)
    if codes.dim() != 2 or not codes.is_contiguous() or not absmax.is_contiguous():
        raise ValueError('dequantize_4bit_t: codes (N, K/2) and absmax (N, K/64) must be contiguous')
    N, K = codes.shape[0], codes.shape[1] * 2
    if absmax.numel() != N * (K // 64):
        raise ValueError(f'dequantize_4bit_t: absmax has {absmax.numel()} entries, expected {N * (K // 64)}')
    out, op, ldo = _out(out, K, N, codes.device, 'dequantize_4bit_t')
    with _hip._Traced('dequant4_t', (N, K)):
        _hip._check(_lib().esme_hip_dequantize_4bit_t(codes.data_ptr(), absmax.data_ptr(), N, K, _hip._codebook_arg(codebook), op, ldo,
                                                      _hip._stream()), 'esme_hip_dequantize_4bit_t')
    return out


def dequantize_8bit_t(codes: torch.Tensor, scale: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(K, N) bf16: out[k, n] = the value _hip.dequantize_8bit(codes, scale) holds at [n, k], bit for bit."""
    _hip._dev(codes, 'dequantize_8bit_t codes', torch.int8)
    _hip._dev(scale, 'dequantize_8bit_t scale', torch.float32)
    if codes.dim() != 2 or not codes.is_contiguous() or scale.numel() != codes.shape[0] or not scale.is_contiguous():
        raise ValueError('dequantize_8bit_t: codes (N, K) and scale (N,) must be contiguous')
    N, K = codes.shape
    out, op, ldo = _out(out, K, N, codes.device, 'dequantize_8bit_t')
    with _hip._Traced('dequant8_t', (N, K)):
        _hip._check(_lib().esme_hip_dequantize_8bit_t(codes.data_ptr(), scale.data_ptr(), N, K, op, ldo, _hip._stream()),
                    'esme_hip_dequantize_8bit_t')
    return out
