"""ctypes binding of include/esme_hip_optim.h (csrc/optim.hip): the fused AdamW step with fp32 master weights over a tensor list, the
global gradient norm and the fp32 gradient accumulator.

The entry points live in a header of their own, so they have a signature table of their own; every call goes through
`_hip.load()`, the one handle of libesme_hip.so (a recorder installed over `_hip._lib` sees these calls too).

Every entry point reads a table (`Table`): rows {param, grad, master, exp_avg, exp_avg_sq, numel, flags, group, step_size,
inv_sqrt_bc2}, per-group hyperparameters and the prefix of chunk counts.  It is filled on the host (numpy, `fill_table`), uploaded by
one stream-ordered copy, and handed to the library twice: the host bytes are validated there before anything launches."""
from __future__ import annotations

import ctypes
import math
from ctypes import c_float, c_int, c_int64, c_void_p
from typing import Optional, Sequence

import numpy as np
import torch

from esme import _hip

SIGNATURES = {
    'esme_hip_optim_chunk_elems': (c_int, []),
    'esme_hip_optim_table_bytes': (c_int64, [c_int, c_int]),
    'esme_hip_optim_workspace_bytes': (c_int64, [c_int64]),
    'esme_hip_optim_adamw_step': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'esme_hip_optim_grad_sqnorm': (c_int, [c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_void_p, c_int64, c_void_p, c_void_p]),
    'esme_hip_optim_grad_accumulate': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
}

CHUNK = 8192                                     # ESME_OPTIM_CHUNK
PARAM_F32, GRAD_F32, ACC_INIT = 1, 2, 4          # ESME_OPTIM_PARAM_F32 / _GRAD_F32 / _ACC_INIT
ROW = np.dtype([('param', '<u8'), ('grad', '<u8'), ('master', '<u8'), ('exp_avg', '<u8'), ('exp_avg_sq', '<u8'), ('numel', '<i8'),
                ('flags', '<i4'), ('group', '<i4'), ('step_size', '<f4'), ('inv_sqrt_bc2', '<f4')])           # esme_optim_row_t
GROUP = np.dtype([(n, '<f4') for n in ('lr', 'beta1', 'beta2', 'eps', 'weight_decay', 'decay', 'one_minus_beta1', 'one_minus_beta2')])      # esme_optim_group_t
assert ROW.itemsize == 64 and GROUP.itemsize == 32


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


def table_bytes(n_tensors: int, n_groups: int) -> int:
    return ROW.itemsize * n_tensors + GROUP.itemsize * n_groups + 8 * (n_tensors + 1)


def chunk_prefix(numels: Sequence[int]) -> np.ndarray:
    """int64 (n + 1): prefix[r + 1] = prefix[r] + ceil(numel[r] / CHUNK).  The chunk map of a list: a function of its numels alone."""
    prefix = np.zeros(len(numels) + 1, dtype=np.int64)
    np.cumsum(-(-np.asarray(numels, dtype=np.int64) // CHUNK), out=prefix[1:])
    return prefix


def workspace_bytes(total_chunks: int) -> int:
    n = _lib().esme_hip_optim_workspace_bytes(int(total_chunks))
    if n < 0:
        _hip._check(n, 'esme_hip_optim_workspace_bytes')
    return int(n)


def group_record(lr: float, beta1: float, beta2: float, eps: float, weight_decay: float) -> tuple:
    """One esme_optim_group_t: the derived scalars are formed in float64 and rounded once to fp32 by the table."""
    return (lr, beta1, beta2, eps, weight_decay, 1.0 - lr * weight_decay, 1.0 - beta1, 1.0 - beta2)


def bias_terms(lr: float, beta1: float, beta2: float, step: int) -> tuple:
    """(step_size, inv_sqrt_bc2) of a tensor at its step count `step` >= 1, in float64."""
    return lr / (1.0 - beta1 ** step), 1.0 / math.sqrt(1.0 - beta2 ** step)


class Table:
    """Views into one host buffer of table_bytes(n, ng) bytes (`buf`: a uint8 numpy array, e.g. of a pinned tensor): .rows (ROW),
    .groups (GROUP), .prefix (int64)."""
    __slots__ = ('buf', 'n', 'ng', 'rows', 'groups', 'prefix')

    def __init__(self, buf: np.ndarray, n: int, ng: int):
        a, b = ROW.itemsize * n, ROW.itemsize * n + GROUP.itemsize * ng
        self.buf, self.n, self.ng = buf, n, ng
        self.rows = buf[:a].view(ROW)
        self.groups = buf[a:b].view(GROUP)
        self.prefix = buf[b:b + 8 * (n + 1)].view(np.int64)

    @property
    def nbytes(self) -> int:
        return table_bytes(self.n, self.ng)

    @property
    def total_chunks(self) -> int:
        return int(self.prefix[self.n])


def fill_table(rows: Sequence[dict], groups: Sequence[tuple], buf: Optional[np.ndarray] = None) -> Table:
    """A Table from row dicts {param, grad, master, exp_avg, exp_avg_sq: addresses (0 / absent: NULL), numel, flags, group, step_size,
    inv_sqrt_bc2} and group_record() tuples: the convenient form, for tests and tools (esme.optim.AdamW writes the columns itself)."""
    n, ng = len(rows), len(groups)
    if buf is None:
        buf = np.zeros(table_bytes(n, ng), dtype=np.uint8)
    t = Table(buf, n, ng)
    for i, r in enumerate(rows):
        t.rows[i] = tuple(r.get(k, 0) or 0 for k in ROW.names)
    for i, g in enumerate(groups):
        t.groups[i] = tuple(g)
    t.prefix[:] = chunk_prefix([r['numel'] for r in rows])
    return t


def upload(table: Table, device) -> tuple:
    """(host uint8 tensor, device uint8 tensor) of the table's bytes: a plain blocking copy, for tests and tools."""
    host = torch.from_numpy(table.buf[:table.nbytes])
    return host, host.to(device)


def _tables(host: torch.Tensor, dev: torch.Tensor, what: str):
    if host.is_cuda or host.dtype != torch.uint8 or not host.is_contiguous():
        raise TypeError(f'{what}: the host table must be a contiguous uint8 CPU tensor')
    if dev.numel() < host.numel():
        raise ValueError(f'{what}: the device table holds {dev.numel()} bytes, the host table {host.numel()}')
    return host.data_ptr(), _hip._dev(dev, f'{what} table', torch.uint8)


def adamw_step(host: torch.Tensor, dev: torch.Tensor, n_tensors: int, n_groups: int, scale: torch.Tensor) -> None:
    """esme_hip_optim_adamw_step on an uploaded table; `scale`: a device float32 tensor of one element."""
    hp, dp = _tables(host, dev, 'optim adamw_step')
    sp = _hip._dev(scale, 'optim adamw_step scale', torch.float32)
    with _hip._Traced('optim_adamw_step', (n_tensors, n_groups)):
        _hip._check(_lib().esme_hip_optim_adamw_step(hp, dp, n_tensors, n_groups, sp, _hip._stream()), 'esme_hip_optim_adamw_step')


def grad_sqnorm(host: torch.Tensor, dev: torch.Tensor, n_tensors: int, n_groups: int, max_norm: float, grad_scale: float,
                out: torch.Tensor, workspace: torch.Tensor) -> None:
    """esme_hip_optim_grad_sqnorm: out (3 float32 on the device) = (norm, clip coefficient, coefficient x grad_scale); `workspace`: a
    uint8 device tensor of at least workspace_bytes(total chunks) bytes."""
    hp, dp = _tables(host, dev, 'optim grad_sqnorm')
    if out.numel() < 3 or not out.is_contiguous():
        raise ValueError('optim grad_sqnorm: out must hold 3 contiguous float32')
    op = _hip._dev(out, 'optim grad_sqnorm out', torch.float32)
    wp = _hip._dev(workspace, 'optim grad_sqnorm workspace', torch.uint8)
    with _hip._Traced('optim_grad_sqnorm', (n_tensors,)):
        _hip._check(_lib().esme_hip_optim_grad_sqnorm(hp, dp, n_tensors, n_groups, float(max_norm), float(grad_scale), wp, workspace.numel(), op,
                                                      _hip._stream()), 'esme_hip_optim_grad_sqnorm')


def grad_accumulate(host: torch.Tensor, dev: torch.Tensor, n_tensors: int, n_groups: int) -> None:
    """esme_hip_optim_grad_accumulate: rows' `master` (the fp32 accumulators) += rows' `grad`."""
    hp, dp = _tables(host, dev, 'optim grad_accumulate')
    with _hip._Traced('optim_grad_accumulate', (n_tensors,)):
        _hip._check(_lib().esme_hip_optim_grad_accumulate(hp, dp, n_tensors, n_groups, _hip._stream()), 'esme_hip_optim_grad_accumulate')
