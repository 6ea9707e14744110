"""The autograd seam of fine-tuning: the nodes whose forward AND backward are this package's kernels.

 - `VarlenAttention`: forward = esme_hip_attn_varlen_fwd on the current stream (the plain form: q not prescaled, bf16), backward =
   esme_hip_attn_varlen_bwd (include/esme_hip_attn_bwd.h).  torch has no stand-in for the backward of block-diagonal attention over a
   cu_lens-packed batch; everything else of a training step is torch.autograd on torch ops.
 - `FrozenLinear`: a projection whose weight does not require grad: forward = the GEMM kernel, backward dX = dY W on the same kernel
   against W^T from the derived-weight cache (esme.nn.weight_t).
 - `TrainableLinear`: a layer's own projection whose weight requires grad (model.mark_trainable): the same forward and dX, and
   (dW, db) = esme_hip_gemm_wgrad (include/esme_hip_gemm_wgrad.h) in bfloat16, the parameters' dtype.
 - `QuantFrozenLinear`: a frozen projection stored as 4-bit / int8 codes (a model that opted in with add_lora(quantized_base=True)):
   W and, in the backward, W^T are expanded from the codes into the model's one weight scratch each time they are used
   (include/esme_hip_dequant_t.h); no bf16 copy of either is kept.
 - `TokenEmbedding`: the token-embedding lookup of a model that opted in with mark_trainable(embedding=True): forward =
   esme_hip_embed, backward = esme_hip_embed_bwd (include/esme_hip_embed_bwd.h): per table row the fp32 sum of its rows of dX in a fixed
   order, without atomics.
 - `PositionEmbedding`: the token + learned-position lookup of an ESM-1b / ESM-1v model that opted in with
   mark_trainable(positions=...): forward = esme_hip_embed_positions on packed ids, backward = esme_hip_embed_bwd for the token table
   and esme_hip_embed_positions_bwd (include/esme_hip_embed_positions_bwd.h) for the position table: per table row the fp32 sum over
   the sequences in ascending order, without atomics.

 - `AttentionPooling`: forward = esme_hip_attn_pool on the folded queries U, backward = esme_hip_attn_pool_bwd
   (include/esme_hip_attn_pool_bwd.h); `pool_fold` is the fold itself in fp32 torch ops, so that autograd carries dU on to the class
   tokens and the key weight.  `SegmentMean`: forward = esme_hip_segment_mean, backward =
   esme_hip_segment_mean_bwd (include/esme_hip_segment_mean_bwd.h): no host read of cu_lens, so the node does not stall the stream.

 - `LinearCrossEntropy`: a linear layer of at most 64 outputs fused with the cross-entropy of its logits over packed rows (the loss of a
   per-residue head and of the masked-LM head's vocabulary projection): forward = esme_hip_linear_xent_fwd, backward =
   esme_hip_linear_xent_bwd (include/esme_hip_linear_xent.h).  The logits are never materialised, the labelled rows are selected
   inside the kernel (no nonzero), the upstream gradient stays on the device: neither direction synchronises with the host.

 - `CRFLogPartition`: log Z of a linear-chain CRF per packed sequence (include/esme_hip_crf.h): forward = esme_hip_crf_fwd (the forward
   algorithm), backward = one call of esme_hip_crf_bwd (the backward algorithm) with the (B,) upstream gradient left on the device.

`forward_trainable` of the attention block, the layer and the model (esme/attention.py, esme/esm.py) is written with the first two and
torch ops, in the reference's unfused data flow; `forward_trainable` of the task heads (esme/pooling.py, esme/head.py) with the pooling
nodes and torch ops.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from esme import (_hip, _hip_attn_bwd, _hip_attn_pool_bwd, _hip_crf, _hip_embed_bwd, _hip_embed_positions_bwd, _hip_gemm_wgrad,
                  _hip_linear_xent, _hip_segment_mean_bwd)
from esme.nn import weight_t


class VarlenAttention(torch.autograd.Function):
    """out (T, H * d) = varlen attention of q, k, v (T, H * d) bfloat16 over the sequences of `cu_lens`."""

    @staticmethod
    def forward(ctx, q, k, v, cu_lens, max_len, heads, softmax_scale):
        T, E = q.shape
        qkv = torch.empty(T, 3 * E, dtype=torch.bfloat16, device=q.device)       # (one row stride: the layout both kernels read)
        for i, t in enumerate((q, k, v)):
            qkv[:, i * E:(i + 1) * E].copy_(t)
        q, k, v = (qkv[:, i * E:(i + 1) * E] for i in range(3))
        if cu_lens.dtype != torch.int32:
            cu_lens = cu_lens.to(torch.int32)
        o = _hip.attn_varlen(q, k, v, cu_lens, int(max_len), int(heads), softmax_scale=float(softmax_scale))
        ctx.save_for_backward(qkv, o, cu_lens)
        ctx.args = (int(max_len), int(heads), float(softmax_scale))
        return o

    @staticmethod
    def backward(ctx, d_o):
        qkv, o, cu_lens = ctx.saved_tensors
        E = o.shape[1]
        if d_o.stride(1) != 1 or d_o.stride(0) % 8 or d_o.data_ptr() % 16:
            d_o = d_o.contiguous()
        max_len, heads, scale = ctx.args
        dq, dk, dv = _hip_attn_bwd.attn_varlen_bwd(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], o, d_o, cu_lens, max_len, heads, scale)
        return dq, dk, dv, None, None, None, None


class TokenEmbedding(torch.autograd.Function):
    """x (T, E) = the rows table[tokens] for packed int64 ids (T,), zero rows for `mask_idx` / `pad_idx` (-1: none) and for ids outside
    the table; differentiable in `table` (V, E) bfloat16.  The excluded rows of the table get a zero gradient: they do not reach x."""

    @staticmethod
    def forward(ctx, table, tokens, mask_idx, pad_idx):
        tokens = tokens.contiguous()
        ctx.save_for_backward(tokens)
        ctx.args = (table.shape[0], int(mask_idx), int(pad_idx))
        return _hip.embed(tokens, table.detach(), mask_idx=int(mask_idx), pad_idx=int(pad_idx))

    @staticmethod
    def backward(ctx, d_x):
        tokens, = ctx.saved_tensors
        V, mask_idx, pad_idx = ctx.args
        return _hip_embed_bwd.embed_bwd(_kernel_rows(d_x), tokens, V, mask_idx, pad_idx), None, None, None


class PositionEmbedding(torch.autograd.Function):
    """x (T, E) = table[tokens] (zero rows for `mask_idx` and for ids outside the table) + pos_table[in-sequence position + pos_offset]
    for packed int64 ids (T,) and the sequences of `cu_lens` (int32), the sum rounded to bfloat16 once: the bits of the inference
    embedding of the same rows.  Differentiable in `table` (V, E) and `pos_table` (P, E), both bfloat16; the two addends share one
    gradient, so d_x feeds both backward kernels unchanged, each only where its table takes a gradient."""

    @staticmethod
    def forward(ctx, table, pos_table, tokens, cu_lens, max_len, mask_idx, pos_offset):
        tokens = tokens.contiguous()
        if cu_lens.dtype != torch.int32:
            cu_lens = cu_lens.to(torch.int32)
        cu_lens = cu_lens.contiguous()
        ctx.save_for_backward(tokens, cu_lens)
        ctx.args = (table.shape[0], pos_table.shape[0], int(max_len), int(mask_idx), int(pos_offset))
        pos, _ = _hip.seq_positions(cu_lens, tokens.numel())
        return _hip.embed_positions(tokens, table.detach(), pos_table.detach(), pos, int(pos_offset), mask_idx=int(mask_idx))

    @staticmethod
    def backward(ctx, d_x):
        tokens, cu_lens = ctx.saved_tensors
        V, P, max_len, mask_idx, pos_offset = ctx.args
        d_x = _kernel_rows(d_x)
        d_table = _hip_embed_bwd.embed_bwd(d_x, tokens, V, mask_idx, -1) if ctx.needs_input_grad[0] else None
        d_pos = _hip_embed_positions_bwd.embed_positions_bwd(d_x, cu_lens, P, pos_offset, max_len) if ctx.needs_input_grad[1] else None
        return d_table, d_pos, None, None, None, None, None


class FrozenLinear(torch.autograd.Function):
    """y = x W^T + b on the GEMM kernel for a W that takes no gradient; dX = dY W on the same kernel (`wt` = W^T, contiguous)."""

    @staticmethod
    def forward(ctx, x, w, b, wt):
        ctx.wt = wt
        return _hip.gemm(x if x.stride(-1) == 1 else x.contiguous(), w, b)

    @staticmethod
    def backward(ctx, dy):
        if dy.stride(1) != 1 or dy.stride(0) % 8 or dy.data_ptr() % 16:
            dy = dy.contiguous()
        return _hip.gemm(dy, ctx.wt), None, None, None


def _kernel_rows(t: torch.Tensor) -> torch.Tensor:
    """t as the GEMM kernels read a 2-D operand: unit column stride, a row stride that is a multiple of 8, a 16-byte aligned base."""
    if t.stride(1) != 1 or t.stride(0) % 8 or t.data_ptr() % 16:
        t = t.contiguous()
    return t


class TrainableLinear(torch.autograd.Function):
    """y = x W^T + b on the GEMM kernel for a projection `lin` that is trained: dX = dY W on the same kernel (W^T from
    esme.nn.weight_t, whose key holds the weight's version counter: it is rebuilt after an optimiser step), dW = dY^T X and
    db = the column sums of dY on esme_hip_gemm_wgrad, in bfloat16."""

    @staticmethod
    def forward(ctx, x, w, b, lin):
        x = _kernel_rows(x.detach())
        ctx.save_for_backward(x, w)
        ctx.lin, ctx.has_bias = lin, b is not None
        return _hip.gemm(x, w, b)

    @staticmethod
    def backward(ctx, dy):
        x, _ = ctx.saved_tensors
        dy = _kernel_rows(dy)
        dx = _hip.gemm(dy, weight_t(ctx.lin)) if ctx.needs_input_grad[0] else None
        dw = db = None
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_b:
            dw, db = _hip_gemm_wgrad.gemm_wgrad(dy, x, bias=want_b)
        return dx, (dw if ctx.needs_input_grad[1] else None), db, None


class QuantFrozenLinear(torch.autograd.Function):
    """y = x W^T + b for a quantised projection `qlin` (esme.quantization.Linear4bit / Linear8bit), which takes no gradient: the forward
    expands W from the codes into `scratch` (the model's one WeightScratch) and runs the GEMM kernel on it; the backward expands W^T
    from the same codes (esme_hip_dequantize_*_t) into the same buffer and runs dX = dY W on the same kernel against it.  Nothing of weight
    size is saved or cached: the context holds references to the module and the scratch only.

    One buffer suffices because an expansion and the GEMM that consumes it are enqueued back to back on one stream: whatever is
    expanded next (another projection's forward, a recomputed forward under checkpoint_layers=True in the middle of the backward)
    is ordered after that GEMM.  This rests on every launch going to ONE stream, so the backward refuses to run on another one
    than the forward's (autograd runs a node's backward on its forward's stream; the check names what broke if that ever changes)."""

    @staticmethod
    def forward(ctx, x, qlin, scratch):
        N, K = qlin.out_features, qlin.in_features
        w = qlin.dequantize(out=scratch.view(N, K, x.device))
        ctx.qlin, ctx.scratch, ctx.stream = qlin, scratch, _hip._stream()
        return _hip.gemm(x if x.stride(-1) == 1 else x.contiguous(), w, qlin.bias)

    @staticmethod
    def backward(ctx, dy):
        qlin = ctx.qlin
        if _hip._stream() != ctx.stream:
            raise RuntimeError('QuantFrozenLinear: the backward runs on another stream than the forward; the shared weight scratch is '
                               'ordered by ONE stream (run forward_trainable and backward under the same torch.cuda.stream)')
        dy = _kernel_rows(dy)
        wt = qlin.dequantize_t(out=ctx.scratch.view(qlin.in_features, qlin.out_features, dy.device))
        return _hip.gemm(dy, wt), None, None


class AttentionPooling(torch.autograd.Function):
    """out (B, n_cls, E) = attention pooling of embed (T, E) bfloat16 / float32 with the folded queries U (n_cls * heads, E) float32
    (`pool_fold`); differentiable in embed and U."""

    @staticmethod
    def forward(ctx, embed, cu_lens, U, heads, n_cls):
        if cu_lens.dtype != torch.int32:
            cu_lens = cu_lens.to(torch.int32)
        embed, U = embed.detach(), U.detach().contiguous()
        if embed.stride(-1) != 1:
            embed = embed.contiguous()
        ctx.save_for_backward(embed, U, cu_lens)
        ctx.args = (int(heads), int(n_cls))
        return _hip.attn_pool(embed, cu_lens, U, int(heads), int(n_cls))

    @staticmethod
    def backward(ctx, d_out):
        embed, U, cu_lens = ctx.saved_tensors
        heads, n_cls = ctx.args
        dx, dU = _hip_attn_pool_bwd.attn_pool_bwd(embed, cu_lens, U, d_out.contiguous(), heads, n_cls, need_dx=ctx.needs_input_grad[0])
        return dx, None, (dU if ctx.needs_input_grad[2] else None), None, None


def pool_fold(cls: torch.Tensor, k_weight: torch.Tensor, heads: int) -> torch.Tensor:
    """U (n_cls * heads, E) float32 = log2(e) / sqrt(d) * W_k[h d:(h+1) d, :]^T cls[c, h d:(h+1) d] in fp32 torch ops: what
    esme_hip_attn_pool_fold computes (to fp32 rounding), differentiable in cls and k_weight."""
    C, E = cls.shape
    d = E // heads
    scale = 1.4426950408889634 / math.sqrt(d)                       # (rounded to fp32 by the product, as the kernel's)
    u = torch.einsum('chd,hde->che', cls.float().view(C, heads, d), k_weight.float().view(heads, d, E))
    return (u * scale).reshape(C * heads, E)


class SegmentMean(torch.autograd.Function):
    """(B, E) per-sequence mean of the rows of x (T, E) bfloat16 / float32 (esme_hip_segment_mean); backward dY[seg] / len
    (fp32 division, one rounding to x's dtype; zero rows outside the sequences) on esme_hip_segment_mean_bwd, without a host
    synchronisation."""

    @staticmethod
    def forward(ctx, x, cu_lens):
        if cu_lens.dtype != torch.int32:
            cu_lens = cu_lens.to(torch.int32)
        ctx.save_for_backward(cu_lens)
        ctx.rows = x.shape[0]
        x = x.detach()
        return _hip.segment_mean(x if x.stride(-1) == 1 else x.contiguous(), cu_lens)

    @staticmethod
    def backward(ctx, dy):
        cu_lens, = ctx.saved_tensors
        if dy.stride(1) != 1 or (dy.stride(0) * dy.element_size()) % 16 or dy.data_ptr() % 16:
            dy = dy.contiguous()
        return _hip_segment_mean_bwd.segment_mean_bwd(dy, cu_lens, ctx.rows), None


class LinearCrossEntropy(torch.autograd.Function):
    """The float32 device scalar  sum_t l_t  (`mean` False) or  sum_t l_t / sum_kept cw[y_t]  (`mean` True; 0 when no weight is kept,
    where torch returns NaN) with l_t = cw[y_t] (logsumexp(x_t w^T + b) - (x_t w^T + b)[y_t]) on the rows whose label is neither
    `ignore_index` nor outside [0, C), and 0 on the others.  x (T, E), w (C, E), b (C) or None in bfloat16, labels (T,) int32 / int64,
    class_weight (C,) float32 or None.  Differentiable in x, w and b; dw and db are rounded to bfloat16 once."""

    @staticmethod
    def forward(ctx, x, w, b, labels, ignore_index, class_weight, mean):
        x, w = _kernel_rows(x.detach()), _kernel_rows(w.detach())
        b = None if b is None else b.detach().contiguous()
        labels = labels.contiguous()
        if labels.data_ptr() % 16:
            labels = labels.clone()
        sums, _, lse = _hip_linear_xent.linear_xent_fwd(x, w, b, labels, ignore_index, class_weight, mean)
        ctx.save_for_backward(x, w, b, labels, class_weight, lse, sums)
        ctx.args = (int(ignore_index), bool(mean))
        return sums[2].clone()                                    # (its own storage: an in-place op on the loss leaves `sums` alone)

    @staticmethod
    def backward(ctx, g):
        x, w, b, labels, class_weight, lse, sums = ctx.saved_tensors
        ignore_index, mean = ctx.args
        g = g.to(torch.float32).reshape(1)
        if g.data_ptr() % 16:
            g = g.clone()
        want_dx = ctx.needs_input_grad[0]
        want_dw = ctx.needs_input_grad[1] or (b is not None and ctx.needs_input_grad[2])
        dx = dw = db = None
        if want_dx or want_dw:
            dx, dw, db = _hip_linear_xent.linear_xent_bwd(x, w, b, labels, lse, sums, g, ignore_index, class_weight, mean,
                                                          want_dx=want_dx, want_dw=want_dw)
        return (dx, dw if ctx.needs_input_grad[1] else None, db if (b is not None and ctx.needs_input_grad[2]) else None,
                None, None, None, None)


def _f32_rows(t: torch.Tensor) -> torch.Tensor:
    """t (T, C) as the CRF kernels read it: float32, unit column stride, a 16-byte aligned base."""
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    if t.stride(1) != 1 or t.data_ptr() % 16:
        t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class CRFLogPartition(torch.autograd.Function):
    """logz (B,) float32: per sequence of `cu_lens` the log of the summed exponentiated scores of every label path that `tags` allows
    (int32 (T,): a label in [0, C) constrains its row, esme._hip_crf.FREE leaves it free, anything else takes the row out of the
    chain; an empty chain gives 0).  emissions (T, C); transitions (C, C) with [i][j] the score of moving from i to j, start, end (C,).
    Differentiable in the first four, all in float32; neither direction synchronises with the host."""

    @staticmethod
    def forward(ctx, emissions, transitions, start, end, tags, cu_lens):
        ctx.e_dtype = emissions.dtype
        e = _f32_rows(emissions)
        A, s, n = (t.detach().float().contiguous() for t in (transitions, start, end))
        tags = tags.to(torch.int32).contiguous()
        cu_lens = cu_lens.to(torch.int32).contiguous()
        logz, alpha = _hip_crf.crf_fwd(e, A, s, n, cu_lens, tags)
        ctx.save_for_backward(e, A, s, n, tags, cu_lens, alpha, logz)
        return logz.clone()                                       # (its own storage: an in-place op on the result leaves the saved logz alone)

    @staticmethod
    def backward(ctx, g):
        e, A, s, n, tags, cu_lens, alpha, logz = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        if g.data_ptr() % 16:
            g = g.clone()
        want = any(ctx.needs_input_grad[1:4])
        d_e, d_t, d_s, d_n = _hip_crf.crf_bwd(e, A, s, n, cu_lens, tags, alpha, logz, g, want_params=want)
        pick = lambda i, t: t if (t is not None and ctx.needs_input_grad[i]) else None
        return (pick(0, d_e.to(ctx.e_dtype)), pick(1, d_t), pick(2, d_s), pick(3, d_n), None, None)


def relu_mlp(x: torch.Tensor, lin, final) -> torch.Tensor:
    """final(relu(lin(x))) in torch ops on the modules' own parameters: the part of a task head that is trained."""
    w = (lambda p: p) if x.dtype == torch.bfloat16 else (lambda p: p.to(x.dtype))     # (a float32 embedding: the bf16 values in fp32 ops)
    return F.linear(F.relu(F.linear(x, w(lin.weight), w(lin.bias))), w(final.weight), w(final.bias))


def check_head_input(x: torch.Tensor, params, what: str) -> None:
    """What the task heads' forward_trainable serves: bfloat16 parameters and a bfloat16 or float32 embedding on a HIP device."""
    if x.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f'{what}: embed must be bfloat16 or float32, got {x.dtype}')
    for n, p in params:
        refuse(p.dtype != torch.bfloat16, f'{what}: parameter {n} is {p.dtype}; the heads keep bfloat16 parameters')


def frozen_linear(x: torch.Tensor, lin, layer_projection: bool = False) -> torch.Tensor:
    """lin(x) for a 2-D bfloat16 x, differentiable in x (and in lin's parameters where they require grad).  The kernels serve a
    bfloat16 projection whose two widths are multiples of 64 (the GEMM's K tile, the weight-gradient kernel's wave tile): frozen, it is
    `FrozenLinear` (`QuantFrozenLinear` when it is stored quantised); trained (model.mark_trainable) and one of a layer's own projections (`layer_projection`: q, k, v, out, FFN up /
    down, SwiGLU's two), it is `TrainableLinear`.  Any other trainable projection (the LM head after mark_lmhead) and any other shape
    (the vocabulary projection: dX = dY W has K = vocab_size) is torch's F.linear."""
    if _is_quantised(lin):                                # (check_linear let it through: the model opted in)
        refuse(getattr(lin, 'scratch', None) is None, 'a quantised projection outside a quantised model has no weight scratch (quantize_model_ sets it)')
        return QuantFrozenLinear.apply(x, lin, lin.scratch)
    w, b = lin.weight, lin.bias
    trainable = w.requires_grad or (b is not None and b.requires_grad)
    if w.shape[0] % 64 or w.shape[1] % 64 or (trainable and not layer_projection):
        return F.linear(x, w, b)
    if trainable:
        return TrainableLinear.apply(x, w, b, lin)
    return FrozenLinear.apply(x, w, b, weight_t(lin))


def lora_linear(x: torch.Tensor, mod, names) -> torch.Tensor:
    """The projection `mod` (an esme.nn.Linear, or an esme.lora.LoRA around one) with the adapters `names` selects:
    base(x) + sum_n scaling * (x A_n^T) B_n^T, the delta in torch ops (the gradients of A_n and B_n are torch's)."""
    from esme.lora import LoRA
    if not isinstance(mod, LoRA):
        return frozen_linear(x, mod, True)
    y = frozen_linear(x, mod.layer, True)
    for n in mod.select(names):
        y = y + F.linear(F.linear(x, mod.lora_A[n]), mod.lora_B[n]) * mod.scaling
    return y


def layer_norm(x: torch.Tensor, ln) -> torch.Tensor:
    return F.layer_norm(x, (x.shape[-1],), ln.weight, ln.bias, ln.eps)


def rotate_half(x: torch.Tensor) -> torch.Tensor:
    x1, x2 = x.chunk(2, dim=-1)
    return torch.cat((-x2, x1), dim=-1)


def rotary(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, heads: int) -> torch.Tensor:
    """x (T, H * d) rotated with the tables (max_len, d) at the rows' positions, in torch ops: autograd's backward is the inverse
    rotation (the reference's hand-written backward applies the forward rotation again: DESIGN.md section 8)."""
    T, E = x.shape
    x3 = x.view(T, heads, E // heads)
    c, s = cos[pos].unsqueeze(1), sin[pos].unsqueeze(1)
    return (x3 * c + rotate_half(x3) * s).reshape(T, E)


def pad_rows(x: torch.Tensor, indices: torch.Tensor, batch: int, seqlen: int) -> torch.Tensor:
    """`pad_input` in torch ops: packed rows scattered into zeros, (B, S, C)."""
    out = torch.zeros(batch * seqlen, x.shape[-1], dtype=x.dtype, device=x.device)
    return out.index_copy(0, indices.to(torch.int64), x).view(batch, seqlen, x.shape[-1])


def refuse(cond: bool, what: str) -> None:
    if cond:
        raise NotImplementedError(f'forward_trainable: {what}')


QLORA_HINT = 'adapters train over a quantised base after model.add_lora(quantized_base=True)'


def _is_quantised(lin) -> bool:
    from esme.quantization import Linear4bit, Linear8bit
    return isinstance(lin, (Linear4bit, Linear8bit))


def check_linear(lin, what: str, qlora: bool = False) -> None:
    """Quantised storage has a backward (QuantFrozenLinear) only where the model opted in (`qlora`): name it otherwise."""
    if qlora and _is_quantised(lin):
        return
    refuse(lin.weight.dtype != torch.bfloat16, f'{what} is stored quantised ({lin.weight.dtype}); training needs unquantised bfloat16 base weights ({QLORA_HINT})')


def check_frozen_norms(norms, qlora: bool) -> None:
    """On a quantised base the LayerNorms stay frozen: the quantised matrices of the fused inference forward snapshot the LayerNorm
    gain and the folded constants c1 / c2 when they are built (esme.quantization.Q4Matrix), so a trained LayerNorm would leave
    model.eval(); model(...) stale.  `norms`: (name, module) pairs."""
    if not qlora:
        return
    for name, ln in norms:
        for pn, p in ln.named_parameters(recurse=False):
            refuse(p.requires_grad, f'{name}.{pn} requires grad on a quantised base: the quantised inference forward keeps a snapshot of the '
                   'LayerNorms, so only the adapters and the LM head (mark_lmhead) train here')
