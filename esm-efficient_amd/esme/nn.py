"""Parameter containers whose forward is a HIP kernel (no torch arithmetic).

They keep the reference's parameter names (`weight`, `bias`) so checkpoints in
the reference layout load with `load_state_dict`, but `forward` goes through
the C ABI (`esme._hip`).
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import nn

from esme import _hip


# Parameter epoch: bumped whenever a parameter OBJECT of one of these modules is (re)assigned -- `lin.weight = nn.Parameter(...)`,
# `load_state_dict(assign=True)`, a module swap -- and by `ESM2._apply` / `load_state_dict` / `set_precision` / `invalidate_graphs`.
# Consumers that cache derived weights (esme.cforward.ModelDescriptor) compare it in O(1) instead of walking the module tree.
_EPOCH = [0]


def bump_epoch() -> None:
    _EPOCH[0] += 1


def param_epoch() -> int:
    return _EPOCH[0]


# Weight-edit epoch: bumped by ESM2.invalidate_graphs() (and so by load_state_dict / `.to()`), the documented step after writing weights in place --
# through `p.data` in particular, which moves no version counter.  version_key mixes it into EVERY derived-weight cache key (LN-folded,
# fp16, extension-tile, packed, padded copies), so that no cache can be left out of an invalidation.  Global: another model's caches rebuild once too.
_WEIGHTS_EPOCH = [0]


def bump_weights_epoch() -> None:
    _WEIGHTS_EPOCH[0] += 1


def weights_epoch() -> int:
    return _WEIGHTS_EPOCH[0]


def version_key(*params):
    """Cache key of a copy derived from `params`: their addresses and version counters, and the weight-edit epoch (weights_epoch: moved
    by ESM2.invalidate_graphs after in-place writes that bump no version counter)."""
    return (weights_epoch(),) + tuple((p.data_ptr(), p._version) for p in params if p is not None)


def pad_last(t: Optional[torch.Tensor], n: int) -> Optional[torch.Tensor]:
    """Zero-pad the last dim of a weight / vector to n."""
    if t is None or t.shape[-1] == n:
        return t
    out = torch.zeros(*t.shape[:-1], n, dtype=t.dtype, device=t.device)
    out[..., :t.shape[-1]] = t
    return out


def pad_rows(t: torch.Tensor, n: int) -> torch.Tensor:
    if t.shape[0] == n:
        return t
    out = torch.zeros(n, *t.shape[1:], dtype=t.dtype, device=t.device)
    out[:t.shape[0]] = t
    return out


def flatten_tensors(x):
    """Every tensor inside nested tuples / lists / dicts."""
    if isinstance(x, torch.Tensor):
        yield x
    elif isinstance(x, (tuple, list)):
        for y in x:
            yield from flatten_tensors(y)
    elif isinstance(x, dict):
        for y in x.values():
            yield from flatten_tensors(y)


class Derived:
    """The derived tensors of ONE owner (packed, LayerNorm-folded, fp16, extension-tile, padded, adapter forms of its weights; rotary tables):
    name -> (key, value).  Everything its kernels read that is neither an input nor a parameter lives here or in another object with
    `tensors()`, so esme.graph.external_tensors finds it without knowing names."""
    __slots__ = ('_entries',)

    def __init__(self):
        self._entries = {}

    def get(self, name, key, build, *args, rekey=None):
        """The value cached under `name` if it was built for `key`, else build(*args) (under no_grad), stored.  `rekey`: forms the key to
        store AFTER the build, for a builder that moves the tensors the key is made of.  (On the forward path: a hit costs one dict lookup
        and the comparison, so callers pass a function and its arguments rather than a closure made per call.)"""
        e = self._entries.get(name)
        if e is not None and e[0] == key:
            return e[1]
        with torch.no_grad():
            value = build(*args)
        self._entries[name] = (key if rekey is None else rekey(), value)
        return value

    def key(self, name):
        e = self._entries.get(name)
        return None if e is None else e[0]

    def clear(self, *names):
        for n in names or tuple(self._entries):
            self._entries.pop(n, None)

    def tensors(self):
        for _, value in self._entries.values():
            yield from flatten_tensors(value)


def weight_t(lin) -> torch.Tensor:
    """W^T (in, out), contiguous, of a projection: the weight operand of dX = dY W on the GEMM kernel (esme.autograd.FrozenLinear).
    Cached on the projection itself under a name of its own ('wt'), keyed like every derived copy on the weight's address, version
    counter and the weight-edit epoch: building it leaves the derived weights of the inference paths (which live on the attention
    block and the layer) in place, and it is rebuilt after the QKV pack moves the weight."""
    d = lin.__dict__.get('_derived')
    if d is None:
        d = lin.__dict__['_derived'] = Derived()
    w = lin.weight
    return d.get('wt', version_key(w), _transposed, w)


def _transposed(w):
    return w.data.t().contiguous()


class _TrackedModule(nn.Module):
    def __setattr__(self, name, value):
        if name in ('weight', 'bias'):
            bump_epoch()
        super().__setattr__(name, value)

    def _apply(self, fn, *a, **kw):
        """`.to()` / `.cuda()` / dtype casts on a SUBMODULE move its storage without going through ESM2._apply: bump the epoch here too, so
        that descriptors holding raw pointers to copies derived from the old storage are rebuilt."""
        out = super()._apply(fn, *a, **kw)
        bump_epoch()
        return out


class Linear(_TrackedModule):
    """y = x W^T + b on the bf16 MFMA GEMM (replaces nn.Linear on the path)."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True, dtype=torch.bfloat16, device=None):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features, dtype=dtype, device=device),
                                   requires_grad=False)
        self.bias = nn.Parameter(torch.empty(out_features, dtype=dtype, device=device),
                                 requires_grad=False) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        if self.weight.is_meta:
            return
        bound = 1.0 / math.sqrt(self.in_features)
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)
            if self.bias is not None:
                self.bias.uniform_(-bound, bound)

    def forward(self, x, epilogue=_hip.EPI_NONE, resid=None, alpha=1.0, out=None):
        shape = x.shape
        y = _hip.gemm(x.reshape(-1, shape[-1]), self.weight, self.bias, epilogue, resid, alpha, out)
        return y if x.dim() == 2 else y.view(*shape[:-1], y.shape[-1])

    def extra_repr(self):
        return f'in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}'


class LayerNorm(_TrackedModule):
    """Row LayerNorm over the last dim (fp32 statistics inside the kernel)."""

    def __init__(self, dim: int, eps: float = 1e-5, bias: bool = True, dtype=torch.bfloat16, device=None):
        super().__init__()
        self.dim, self.eps = dim, eps
        self.weight = nn.Parameter(torch.ones(dim, dtype=dtype, device=device), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(dim, dtype=dtype, device=device), requires_grad=False) if bias else None

    def forward(self, x, out=None):
        return _hip.layernorm(x, self.weight, self.bias, self.eps, out)

    def extra_repr(self):
        return f'{self.dim}, eps={self.eps}, bias={self.bias is not None}'


class GELU(nn.Module):
    """Placeholder that keeps the reference's `final.2` slot: the exact-erf GELU is
    fused into the preceding GEMM's epilogue, so this module is never called on the
    packed path."""

    def forward(self, x):  # pragma: no cover
        raise RuntimeError('GELU is fused into the GEMM epilogue (ESME_EPI_GELU)')
