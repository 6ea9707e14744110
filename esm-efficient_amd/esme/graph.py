"""hipGraph replay of the packed forward for a fixed input shape.

A forward of a 30-layer model is ~160 kernel launches through ctypes; below ~10 ms of GPU work the
host cannot enqueue them fast enough (measured: ESM2-150M on 8 192 residues needs 6 ms of GPU time
and 9 ms of Python).  All launches go to the current HIP stream with caller-owned buffers, so a
forward with a fixed `(T, n_sequences, max_len)` can be stream-captured once into a hipGraph
(`torch.cuda.CUDAGraph`, which on ROCm records hipGraph nodes) and replayed with one launch:
`tokens` and `cu_lens` live in static device buffers that are overwritten before each replay.

The shape key includes `max_len` (it sets the attention grid) and the number of sequences (it
sizes `cu_lens`); batches of masked copies of one protein (`esme.variant`) and fixed-size
benchmark batches repeat their shape, token-budget FASTA batches generally do not -- those stay on
the eager path.
"""
from __future__ import annotations

from collections import OrderedDict

import torch

# Device tensors a kernel reads that are not its inputs (packed / LayerNorm-folded / padded weight copies, rotary tables, quantised codes
# and their expansion scratch, the state of precision 'half') are allocated outside a graph's private pool and read by the captured kernels
# through raw pointers.  One rule finds them: besides parameters and buffers, each lives in an object that is an attribute of some module
# and enumerates its tensors with `tensors()` (esme.nn.Derived and the plain state objects alike); no name is listed here.


def external_tensors(model):
    """Every tensor a forward of `model` reads that lives outside the capture pool: the parameters and buffers, and the tensors of
    every attribute of every module that offers `tensors()`.  A captured graph keeps strong references to them: their owners REPLACE
    such tensors (the rotary tables and the quantised layers' scratch regrow when a longer batch or a larger matrix arrives; weight
    copies are rebuilt after a parameter update) and the replaced ones would otherwise be freed while an older graph still holds
    their addresses."""
    keep = [p.data for p in model.parameters()]
    keep.extend(model.buffers())
    for m in model.modules():
        for v in vars(m).values():
            if callable(getattr(v, 'tensors', None)):
                keep.extend(v.tensors())
    return keep


class GraphedForward:
    def __init__(self, model, what: str, n_tokens: int, n_seqs: int, max_len: int, device):
        self.fn = getattr(model, what)
        self.max_len = int(max_len)
        self.tokens = torch.zeros(n_tokens, dtype=torch.int64, device=device)
        self.cu_lens = torch.zeros(n_seqs + 1, dtype=torch.int32, device=device)
        self.model = model
        self.graph = None
        self.out = None
        self._keep = None           # strong references to everything captured from outside the graph's pool

    def _capture(self):
        # run() has copied the caller's batch into the static buffers: the warm-up forwards run on it, and what the plan guard
        # (esme.attention.HalfGuard) records there is data like any other -- merged into the running maxima, not cleared, so that a
        # stale plan seen by an earlier unchecked forward is still reported by the next check.  The inline checks of precision 'half'
        # (predict_log_prob's) are deferred meanwhile: a plan widened between warm-up and capture would clear this very entry from the
        # cache; the caller (ESM2.graphed) checks once after the first replay instead.
        with self.model.half_mode.deferring():
            side = torch.cuda.Stream(device=self.tokens.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), torch.no_grad():
                for _ in range(2):          # builds packed / folded weights, rotary tables, kernel attributes
                    self.fn(self.tokens, (self.cu_lens, self.max_len))
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph), torch.no_grad():
                self.out = self.fn(self.tokens, (self.cu_lens, self.max_len))
        self._keep = external_tensors(self.model)           # e.g. the rotary tables of THIS max_len survive a later regrow
        self.graph = graph

    def run(self, tokens: torch.Tensor, cu_lens: torch.Tensor, clone: bool = True) -> torch.Tensor:
        self.tokens.copy_(tokens, non_blocking=True)
        self.cu_lens.copy_(cu_lens, non_blocking=True)
        if self.graph is None:
            self._capture()
        self.graph.replay()
        return self.out.clone() if clone else self.out


class GraphCache:
    """Per-model LRU of captured forwards, keyed by (method, T, n_sequences, max_len)."""

    def __init__(self, model, capacity: int = 8):
        self.model, self.capacity = model, capacity
        self.entries: 'OrderedDict[tuple, GraphedForward]' = OrderedDict()

    def run(self, what: str, tokens: torch.Tensor, pad_args, clone: bool = True) -> torch.Tensor:
        cu_lens, max_len = pad_args
        assert tokens.ndim == 1, 'graph replay serves the packed (1-D tokens) path'
        key = (what, tokens.numel(), cu_lens.numel() - 1, int(max_len), str(tokens.device))
        g = self.entries.get(key)
        if g is None:
            g = GraphedForward(self.model, what, tokens.numel(), cu_lens.numel() - 1, int(max_len), tokens.device)
            self.entries[key] = g
            while len(self.entries) > self.capacity:
                self.entries.popitem(last=False)
        else:
            self.entries.move_to_end(key)
        return g.run(tokens, cu_lens, clone)

    def clear(self):
        """Drop every captured graph (call after changing weights: a graph replays the weight copies it was
        captured with -- memory-safe because it keeps them alive, but stale)."""
        self.entries.clear()
