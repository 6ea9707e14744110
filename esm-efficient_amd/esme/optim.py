"""esme.optim.AdamW: AdamW with fp32 master weights, fp32 moments and fp32 gradient accumulation for the bfloat16 parameters this
package trains, stepped by one fused HIP kernel over the whole parameter list (include/esme_hip_optim.h).

Why not torch.optim.AdamW on the bf16 parameters: a bf16 weight of magnitude 0.05 has an ulp of 2.4e-4, an update at lr = 1e-5 is under
half of it, and about 97 % of the total update rounds away (tests/test_optim_cpu.py pins the figure).  Here the step is taken on an fp32
master copy and the bf16 parameter is its round-to-nearest-even image.

The kernel writes the parameters through raw pointers, which moves no version counter, while every derived weight of the package
(esme.nn.weight_t, the LN-folded / packed / LoRA-extension copies, captured graphs) is keyed on `weight._version`: step() bumps the
counter of every parameter it stepped.  It also remembers the counter it left: a parameter whose counter differs at the next step was
written by someone else (load_lora, load_state_dict, an edit), and its master is re-seeded from the parameter, with a warning.
"""
from __future__ import annotations

import warnings
from itertools import chain
from typing import Optional

import torch
from torch.optim import Optimizer

from esme import _hip, _hip_optim as HO

__all__ = ['AdamW']

_STATE_F32 = ('master', 'exp_avg', 'exp_avg_sq')


class _HostBuffer:
    """One pinned staging buffer and the event of its last upload: it is rewritten only once that copy has completed."""
    __slots__ = ('tensor', 'array', 'event')

    def __init__(self, nbytes):
        self.tensor = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        self.array = self.tensor.numpy()
        self.event = None


class AdamW(Optimizer):
    """AdamW(params_or_groups, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None).

    Parameters are bfloat16 or float32, contiguous, all on one device; param groups carry lr / betas / eps / weight_decay, so
    torch.optim.lr_scheduler.* works unchanged.  Per-parameter state: `step` (a host int), `master` (fp32; absent for fp32 parameters,
    which are their own master), `exp_avg`, `exp_avg_sq` (fp32), created at the parameter's first step with a gradient; a parameter
    whose gradient is None is skipped and its `step` does not advance.  A gradient is in the parameter's dtype or float32.

    max_grad_norm: clip by one global L2 norm over all groups (clip_grad_norm_'s formula), computed on the device; `last_grad_norm` is
    then a 0-d device tensor -- reading it is the caller's synchronisation.  step() itself never synchronises with the host.

    accumulate(): after a micro-batch's backward(), adds every p.grad into an fp32 accumulator and sets p.grad = None; the next step()
    uses the mean over the accumulate() calls since the last step and clears the accumulators.

    Construction, state_dict() and load_state_dict() need no device; step() and accumulate() run on a HIP device only."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None):
        if isinstance(lr, torch.Tensor):
            raise TypeError('esme.optim.AdamW: lr must be a float (the step reads it on the host)')
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f'esme.optim.AdamW: max_grad_norm must be > 0 or None, got {max_grad_norm}')
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm: Optional[torch.Tensor] = None
        self._left = {}            # parameter -> the version counter step() left on it
        self._acc = {}             # parameter -> its fp32 accumulator
        self._acc_live = set()     # parameters whose accumulator holds gradients since the last step
        self._n_acc = 0            # accumulate() calls since the last step
        self._ring = []            # pinned staging buffers
        self._dev_table = None
        self._workspace = None
        self._ones = {}
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    # ------------------------------------------------------------------ construction

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            self._check_group(len(self.param_groups) - 1, group)
        except Exception:
            self.param_groups.pop()
            raise

    def _check_group(self, gi, group):
        lr, (b1, b2), eps, wd = group['lr'], group['betas'], group['eps'], group['weight_decay']
        if isinstance(lr, torch.Tensor) or not lr >= 0.0:
            raise ValueError(f'esme.optim.AdamW: group {gi}: lr must be a float >= 0, got {lr!r}')
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f'esme.optim.AdamW: group {gi}: betas must lie in [0, 1), got {(b1, b2)}')
        if not eps > 0.0:
            raise ValueError(f'esme.optim.AdamW: group {gi}: eps must be > 0, got {eps}')
        if not wd >= 0.0:
            raise ValueError(f'esme.optim.AdamW: group {gi}: weight_decay must be >= 0, got {wd}')
        names = group.get('param_names')
        first = self.param_groups[0]['params'][0]
        for i, p in enumerate(group['params']):
            what = f'group {gi}, parameter {names[i]!r}' if names else f'group {gi}, parameter {i} of shape {tuple(p.shape)}'
            if p.dtype not in (torch.bfloat16, torch.float32):
                raise TypeError(f'esme.optim.AdamW: {what}: dtype {p.dtype}; parameters must be bfloat16 or float32')
            if not p.is_contiguous():
                raise ValueError(f'esme.optim.AdamW: {what}: not contiguous')
            if p.device != first.device:
                raise ValueError(f'esme.optim.AdamW: {what}: on {p.device}, but the first parameter is on {first.device}; one device only')

    # ------------------------------------------------------------------ checkpoints

    def load_state_dict(self, state_dict):
        """Optimizer.load_state_dict casts every floating-point state tensor to the PARAMETER's dtype, which would bring master and
        the moments back as bfloat16: they are taken out before it runs and put back as float32, bit for bit."""
        saved_groups = state_dict['param_groups']
        ids = list(chain.from_iterable(g['params'] for g in saved_groups))
        params = list(chain.from_iterable(g['params'] for g in self.param_groups))
        kept, state = {}, {}
        for k, s in state_dict['state'].items():
            kept[k] = {n: v for n, v in s.items() if n in _STATE_F32}
            state[k] = {n: v for n, v in s.items() if n not in _STATE_F32}
        super().load_state_dict({'state': state, 'param_groups': saved_groups})
        if len(ids) == len(params):
            for k, p in zip(ids, params):
                for n, v in kept.get(k, {}).items():
                    self.state[p][n] = v.detach().to(device=p.device, dtype=torch.float32, copy=True)
        self._left.clear()         # the loaded masters belong to the parameters as they are now
        self._acc_live.clear()
        self._n_acc = 0

    # ------------------------------------------------------------------ the step

    def _staging(self, nbytes):
        for b in self._ring:
            if b.tensor.numel() >= nbytes and (b.event is None or b.event.query()):
                return b
        b = _HostBuffer(max(4096, 2 * nbytes))
        self._ring.append(b)
        return b

    def _upload(self, buf, nbytes, device):
        if self._dev_table is None or self._dev_table.numel() < nbytes or self._dev_table.device != device:
            self._dev_table = torch.empty(max(4096, 2 * nbytes), dtype=torch.uint8, device=device)
        self._dev_table[:nbytes].copy_(buf.tensor[:nbytes], non_blocking=True)
        buf.event = torch.cuda.Event()
        buf.event.record()
        return buf.tensor[:nbytes], self._dev_table

    @staticmethod
    def _check_grad(p, g):
        if g.dtype != p.dtype and g.dtype != torch.float32:
            raise TypeError(f'esme.optim.AdamW: a gradient of dtype {g.dtype} for a {p.dtype} parameter of shape {tuple(p.shape)}; it must be '
                            f'{p.dtype} or float32')
        if g.device != p.device or g.numel() != p.numel():
            raise ValueError(f'esme.optim.AdamW: the gradient of the parameter of shape {tuple(p.shape)} is on {g.device} with {g.numel()} elements')
        return g if g.is_contiguous() else g.contiguous()

    def _init_state(self, p):
        st = self.state[p]
        st['step'] = 0
        if p.dtype == torch.bfloat16:
            st['master'] = p.detach().float()
        st['exp_avg'] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
        st['exp_avg_sq'] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
        return st

    @torch.no_grad()
    def accumulate(self) -> None:
        """Add every p.grad into the parameter's fp32 accumulator (one launch for the whole list) and set p.grad = None."""
        live, grads, rows = [], [], []
        for p in chain.from_iterable(g['params'] for g in self.param_groups):
            if p.grad is None:
                continue
            _hip._dev(p, 'esme.optim.AdamW.accumulate parameter')
            g = self._check_grad(p, p.grad)
            acc = self._acc.get(p)
            if acc is None:
                acc = self._acc[p] = torch.empty(p.numel(), dtype=torch.float32, device=p.device)
            flags = (HO.GRAD_F32 if g.dtype == torch.float32 else 0) | (0 if p in self._acc_live else HO.ACC_INIT)
            rows.append((0, g.data_ptr(), acc.data_ptr(), 0, 0, p.numel(), flags, 0, 0.0, 0.0))
            live.append(p)
            grads.append(g)
        self._n_acc += 1
        if not rows:
            return
        n = len(rows)
        nbytes = HO.table_bytes(n, 0)
        buf = self._staging(nbytes)
        t = HO.Table(buf.array, n, 0)
        t.rows[:] = rows
        t.prefix[:] = HO.chunk_prefix([r[5] for r in rows])
        host, dev = self._upload(buf, nbytes, live[0].device)
        HO.grad_accumulate(host, dev, n, 0)
        for p in live:
            p.grad = None
            self._acc_live.add(p)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        from_acc = self._n_acc > 0
        params, grads, rows, groups, reseeded = [], [], [], [], 0
        for gi, group in enumerate(self.param_groups):
            lr, (b1, b2) = float(group['lr']), group['betas']
            groups.append(HO.group_record(lr, float(b1), float(b2), float(group['eps']), float(group['weight_decay'])))
            for p in group['params']:
                if from_acc:
                    if p.grad is not None:
                        raise RuntimeError('esme.optim.AdamW.step: accumulate() was called since the last step, but a parameter of shape '
                                           f'{tuple(p.shape)} holds a .grad that was not accumulated; call accumulate() after every backward()')
                    g = self._acc[p] if p in self._acc_live else None
                else:
                    g = p.grad
                if g is None:
                    continue
                _hip._dev(p, 'esme.optim.AdamW.step parameter')
                if not from_acc:
                    g = self._check_grad(p, g)
                st = self.state[p]
                if 'exp_avg' not in st:
                    st = self._init_state(p)
                bf16 = p.dtype == torch.bfloat16
                if bf16 and p in self._left and p._version != self._left[p]:
                    st['master'].copy_(p)                      # written by someone else since our last step: the parameter is the truth
                    reseeded += 1
                st['step'] = t = int(st['step']) + 1
                step_size, isbc2 = HO.bias_terms(lr, b1, b2, t)
                flags = (0 if bf16 else HO.PARAM_F32) | (HO.GRAD_F32 if g.dtype == torch.float32 else 0)
                rows.append((p.data_ptr(), g.data_ptr(), st['master'].data_ptr() if bf16 else 0, st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr(),
                             p.numel(), flags, gi, step_size, isbc2))
                params.append(p)
                grads.append(g)
        if reseeded:
            warnings.warn(f'esme.optim.AdamW: {reseeded} parameter(s) were written outside the optimiser since its last step; their fp32 master '
                          'weights were re-seeded from the parameters', RuntimeWarning, stacklevel=2)
        grad_scale = 1.0 / self._n_acc if from_acc else 1.0
        self._acc_live.clear()
        self._n_acc = 0
        if not rows:
            return loss
        device = params[0].device
        n, ng = len(rows), len(groups)
        nbytes = HO.table_bytes(n, ng)
        buf = self._staging(nbytes)
        t = HO.Table(buf.array, n, ng)
        t.rows[:] = rows
        t.groups[:] = groups
        t.prefix[:] = HO.chunk_prefix([r[5] for r in rows])
        host, dev = self._upload(buf, nbytes, device)
        if self.max_grad_norm is not None:
            need = HO.workspace_bytes(t.total_chunks)
            if self._workspace is None or self._workspace.numel() < need or self._workspace.device != device:
                self._workspace = torch.empty(2 * need, dtype=torch.uint8, device=device)
            out = torch.empty(3, dtype=torch.float32, device=device)
            HO.grad_sqnorm(host, dev, n, ng, self.max_grad_norm, grad_scale, out, self._workspace)
            self.last_grad_norm, scale = out[0], out[2:]
        else:
            scale = self._ones.get((device, grad_scale))
            if scale is None:
                scale = self._ones[device, grad_scale] = torch.full((1,), grad_scale, dtype=torch.float32, device=device)
        HO.adamw_step(host, dev, n, ng, scale)
        torch.autograd.graph.increment_version(params)         # the derived-weight caches and captured graphs are keyed on it
        left = self._left
        for p in params:
            left[p] = p._version
        return loss
