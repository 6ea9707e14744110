"""Loader for tests/golden/*.npz (see tests/golden/make_golden.py)."""
import contextlib
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@contextlib.contextmanager
def exact_cpu_gemms(on=True):
    """Within: every CPU GEMM on bf16 / fp32 operands (F.linear, torch.matmul, `@`) is summed in float64 and rounded once to the
    operands' dtype.  The bf16 fixtures are made (tests/golden/make_golden*.py) and checked bit for bit under it: torch's own CPU
    GEMMs accumulate in fp32 in an order that depends on the processor (oneDNN's AMX kernels differ from its AVX-512 ones), which
    moves a bf16 rounding here and there, so without it the bits would hold on one kind of CPU only."""
    if not on:
        yield
        return
    linear, matmul, tmatmul = F.linear, torch.matmul, torch.Tensor.__matmul__

    def exact(a):
        return a.device.type == 'cpu' and a.dtype in (torch.bfloat16, torch.float32)

    def mm(a, b):
        return matmul(a.double(), b.double()).to(a.dtype) if exact(a) else matmul(a, b)

    def lin(x, w, b=None):
        if not exact(x):
            return linear(x, w, b)
        y = matmul(x.double(), w.double().t())
        return (y if b is None else y + b.double()).to(x.dtype)

    F.linear, torch.matmul, torch.Tensor.__matmul__ = lin, mm, mm
    try:
        yield
    finally:
        F.linear, torch.matmul, torch.Tensor.__matmul__ = linear, matmul, tmatmul


def load_golden(name):
    """npz -> dict of torch tensors / python scalars.  uint16 arrays are bf16
    bit patterns (outputs of the reference's bf16 forward) and come back as
    torch.bfloat16.  A model fixture keeps its bf16 arrays in a companion
    `<name>_bf16.npz` (each file stays small); both are merged here."""
    out = {}
    paths = [os.path.join(GOLDEN, name), os.path.join(GOLDEN, name[:-len('.npz')] + '_bf16.npz')]
    for path in paths[:1] + [p for p in paths[1:] if os.path.exists(p)]:
        with np.load(path, allow_pickle=False) as z:
            for k in z.files:
                assert k not in out, (path, k)
                a = z[k]
                if a.dtype == np.uint16:
                    out[k] = torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16)
                elif a.ndim == 0:
                    out[k] = a.item()
                else:
                    out[k] = torch.from_numpy(a.copy())
    return out


def rel_fro(a, b):
    """Frobenius-relative error ||a-b|| / ||b|| in fp64."""
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))
