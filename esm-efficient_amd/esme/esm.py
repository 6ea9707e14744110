"""ESM-2 / ESM-C model assembly and checkpoint loading for the MI355X hot path.

Public surface mirrors the reference (`esme/esm.py`): `ESM.from_pretrained`
(:28-69), `ESM2` (:72-374: embedding, forward_representation, forward,
predict_log_prob, predict_prob, create_model, from_pretrained) and `ESMC`
(:738-913) with the same argument order, defaults, return shapes/dtypes and
assertion/ValueError behaviour, so callers of
`model(tokens, (cu_lens, max_len))` / `predict_log_prob` switch packages without
edits.  Everything arithmetic runs in HIP kernels behind `esme._hip`; a tensor
that is not on a HIP device raises (there is no CPU fallback).

`quantization='4bit'` / `'8bit'` keep the layer projections 4-bit / int8 in HBM (esme/quantization.py).
ESM-1b / ESM-1v (learned positions, no rotary) run on the same kernels (`ESM1b`, `ESM1v`).
LoRA adapters (`add_lora` / `load_lora` / `save_lora`, `lora_names=`) run for inference in precision 'fast' (esme/lora.py).
`predict_contacts` (with `set_contact_head`) reduces the attention maps into contact maps layer by layer (esme/contacts.py); the
reference has no counterpart (flash-attn returns no attention weights).  `attention_maps` writes the maps of chosen layers and
heads themselves out (esme/attention_maps.py).
Training goes through `forward_trainable` (esme/autograd.py): LoRA adapters, the LM head (`mark_lmhead`) and, after `mark_trainable`,
the layers' own projections and LayerNorms (full fine-tuning; `checkpoint_layers=True` is the reference's `checkpointing=`).
Out of scope here: a backward of the fused inference forward (`model.train(); model(...)` raises, and the
constructor's `checkpointing=` with it), int8-activation matmuls, hub download (no network).
"""
from __future__ import annotations

import math
import os
from typing import List, Optional, Sequence, Tuple

import torch
from torch import nn

from esme import _hip, halfmode, lora_fused
from esme.alphabet import Alphabet, Alphabet3
from esme.attention import FlashTransformerLayer, ForwardContext, padded_head_dim
from esme.head import RobertaLMHead
from esme.embedding import LearnedPositionalEmbedding
from esme.nn import Derived, LayerNorm, bump_epoch, bump_weights_epoch, pad_last, version_key
from esme.qk_observer import dense_blocks

model_names = ['esm2_8m', 'esm2_35m', 'esm2_150m', 'esm2_650m', 'esm2_3b', 'esm2_15b',
               'esmc_300m', 'esmc_600m', 'esm1b', 'esm1v']


def _read_metadata(path: str) -> dict:
    from safetensors import safe_open
    with safe_open(path, framework='pt', device='cpu') as f:
        return dict(f.metadata() or {})


class ESM(nn.Module):
    """Dispatcher: picks the model class from the checkpoint's `name` metadata."""

    @staticmethod
    def from_pretrained(path, quantization=None, checkpointing=False, device='cpu'):
        if not os.path.isfile(path):
            # the reference would try the HF hub here (esm.py:42-48); there is no network
            raise ValueError(f'Invalid model name: {path}. Must be a local safetensors file '
                             f'(hub names {model_names} need a download step that is out of scope)')
        name = _read_metadata(path)['name'].split('_')[0]
        if name == 'esm2':
            return ESM2.from_pretrained(path, quantization, checkpointing, device)
        if name == 'esmc':
            return ESMC.from_pretrained(path, quantization, checkpointing, device)
        if name == 'esm1b':
            return ESM1b.from_pretrained(path, quantization, checkpointing, device)
        if name == 'esm1v':
            return ESM1v.from_pretrained(path, quantization, checkpointing, device)
        raise ValueError(f'Invalid model name: {name}. Must be one of {model_names}')


class ESM2(nn.Module):
    alphabet = Alphabet
    vocab_size = 33
    zero_mask_rows = True          # `<mask>` embedding rows are zeroed (esm.py:189)
    fold_layernorm = os.environ.get('ESME_NO_LN_FOLD', '0') != '1'   # LN folded into the QKV / FFN-up GEMMs
    quant_type_4bit = 'fp4'        # codebook of quantization='4bit' (esme.quantization.CODEBOOKS)
    # 'fast': bf16 residual stream (storage at the reference's rounding points).  'high': fp32 residual stream + fp32
    # LayerNorm statistics + exact online softmax, bf16 only at MFMA operands; slower.
    # 'exact': split-operand mode -- every activation feeding a matrix product is a (hi, lo) bf16 pair, fp32 everywhere else;
    # reproduces the reference's fp32 forward (esme/esm.py:132-141 `dtype=`) to ~1e-5, returns fp32.
    # 'half': IEEE fp16 MFMA operands (weights converted once -- exact for bf16 checkpoints; LayerNorm gains folded as powers of two, the rest
    # rides on the stream --, activations rounded to 11 significant bits instead of 8, same MFMA rate), the residual stream as an fp16 pair
    # (22 bits) updated in place by the residual GEMMs, the LM head in split-operand form: fp32 logits within ~4e-4 of the fp32 forward at
    # ~1.1x the time of 'fast'.  A calibration forward switches on, per model, an extension K-tile for massive stream channels and fp16-pair
    # q / k (`half_robust`, `half_plan()`); activations must stay inside fp16's range (|x| < 65 504): `check_overflow()`.
    precision = os.environ.get('ESME_PRECISION', 'fast')
    # all layers + final LayerNorm through ONE C call (esme_hip_forward) instead of ~5 Python-issued launches per layer
    c_forward = os.environ.get('ESME_NO_C_FORWARD', '0') != '1'

    def __init__(self, num_layers: int = 33, embed_dim: int = 1280, attention_heads: int = 20,
                 checkpointing: bool = False, rotary_embedding: bool = True, dropout: float = 0.,
                 dtype=torch.bfloat16):
        super().__init__()
        if dtype != torch.bfloat16:
            raise NotImplementedError('the HIP path computes in bf16 (fp32 accumulate) only')
        if checkpointing:
            raise NotImplementedError('activation checkpointing is a training feature (out of scope)')
        self.num_layers, self.embed_dim, self.attention_heads = num_layers, embed_dim, attention_heads
        # Physical layout: the GEMM walks K in tiles of 64 and the attention kernels know head dims
        # 16/32/64/128, so a model like ESM2-35M (E = 480, d = 24) runs with a 512-wide residual stream
        # (zero pad columns) and 32-wide heads.  The padding lives in derived weight copies only.
        self.phys_dim = (embed_dim + 63) // 64 * 64
        self.head_pad = padded_head_dim(embed_dim // attention_heads)
        self.padded = self.phys_dim != embed_dim or self.head_pad != embed_dim // attention_heads
        self._derived = Derived()                  # the embedding table at the physical width
        self.checkpointing = False
        self.embed_scale = 1
        self.half_mode = halfmode.HalfState()      # precision 'half': plan, guard, range flag (esme.halfmode)
        self.contact_head = None                   # esme.contacts.ContactHead once set_contact_head() / from_pretrained() found one
        self.embed_tokens = nn.Embedding(self.vocab_size, embed_dim, dtype=dtype,
                                         padding_idx=self.alphabet.padding_idx)
        self.embed_tokens.weight.requires_grad_(False)
        self.layers = nn.ModuleList(self._make_layer(rotary_embedding, dropout, dtype)
                                    for _ in range(num_layers))
        for i, layer in enumerate(self.layers):
            layer.self_attn.layer_index = i
        self.emb_layer_norm_after = self._make_final_norm(dtype)
        self.lm_head = RobertaLMHead(embed_dim, self.vocab_size, dtype=dtype, phys_dim=self.phys_dim)

    # -- construction hooks (ESMC overrides) ---------------------------------
    def _make_layer(self, rotary_embedding, dropout, dtype):
        return FlashTransformerLayer(self.embed_dim, 4, self.attention_heads, rotary_embedding=rotary_embedding,
                                     pre_layernorm=False, bias=True, final_activation='gelu',
                                     dropout=dropout, dtype=dtype, phys_dim=self.phys_dim, head_pad=self.head_pad)

    def _make_final_norm(self, dtype):
        return LayerNorm(self.embed_dim, dtype=dtype)

    # -- embedding -----------------------------------------------------------
    def embedding(self, tokens, pad_args=None):
        """Embedding rows; `<mask>` rows zeroed without rescale (esm.py:188-189); for 2-D
        tokens `<pad>` rows are zeroed too (esm.py:191-193)."""
        if tokens.ndim not in (1, 2):
            raise ValueError('tokens must be 1D or 2D')
        x = self._embedding_phys(tokens, pad_args)
        return x[..., :self.embed_dim].contiguous() if self.padded else x

    def _embed_table(self):
        """Embedding table at the physical width (a zero-padded copy for padded layouts)."""
        w = self.embed_tokens.weight
        if not self.padded:
            return w
        return self._derived.get('embed', version_key(w), pad_last, w.data, self.phys_dim)

    # ESME_CHECK_TOKENS=1 (or model.debug_checks = True): every forward validates its token ids on the device first -- one synchronisation per call.
    # The reference's nn.Embedding raises on an id outside the table (esme/esm.py:176-199); esme_hip_embed writes a zero row instead (no trap on the hot
    # path), a silent divergence for CORRUPT input only: check_tokens() is the explicit form, predict_* call it in precision 'half' (they synchronise anyway).
    debug_checks = os.environ.get('ESME_CHECK_TOKENS', '0') == '1'

    def check_tokens(self, tokens):
        """IndexError if a token id lies outside the embedding table (the reference raises there; the HIP lookup returns a zero row).  Synchronises."""
        if tokens.numel() and not torch.cuda.is_current_stream_capturing():
            lo, hi = int(tokens.min()), int(tokens.max())
            if lo < 0 or hi >= self.embed_tokens.weight.shape[0]:
                raise IndexError(f'token id {lo if lo < 0 else hi} is outside the embedding table of {self.embed_tokens.weight.shape[0]} rows')
        return self

    def _embedding_phys(self, tokens, pad_args=None):
        if self.debug_checks:
            self.check_tokens(tokens)
        return _hip.embed(tokens, self._embed_table(),
                          mask_idx=self.alphabet.mask_idx if self.zero_mask_rows else -1,
                          pad_idx=self.alphabet.padding_idx if (tokens.ndim == 2 and self.zero_mask_rows) else -1)

    def _embedding_exact(self, x, tokens, pad_args, pad_indices):
        """fp32 residual stream at the start of the split-operand mode: the (bf16, hence exactly representable) embedding rows."""
        x32 = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        _hip.residual_f32_(x32, x, 1.0, x, None, init=True)
        return x32

    def _c_forward_ok(self, precision: str = 'fast') -> bool:
        from esme.cforward import ModelDescriptor
        return ModelDescriptor.supported(self, precision)

    # precision 'half' on ill-conditioned checkpoints: 'auto' = a calibration forward on synthetic residues
    # decides, once per model, whether massive stream channels get the extension K-tile and whether q / k travel as pairs
    # (esme.attention.HalfPlan); False = the plain form; True = both measures on (the channel list still comes from the calibration).
    half_robust = {'0': False, '1': True}.get(os.environ.get('ESME_HALF_ROBUST', 'auto'), 'auto')
    HALF_CHANNEL_RATIO = 6.0       # a channel is "massive" when its largest |value| at some stream site exceeds this multiple of the median channel's largest |value| there
    HALF_SCORE_BOUND = 32.0        # q / k become pairs when max |q_i| max |k_j| / sqrt(d) reaches this (2^-12 relative x that = 1e-2 of a score unit)
    HALF_QP_BOUND = 16.0           # the fp16 attention kernel runs its fixed-reference form (P = 2^(score log2(e) - 4), no maximum: HalfPlan.qp) when every layer's calibrated
                                   # bound max |q_i| max |k_j| / sqrt(d) stays below this: a score above the form's 13.9 then needs q and k within 30 degrees of parallel AT
                                   # their largest norms; a work item that gets there anyway is redone with exact maxima by the kernel (correct either way: speed only)
    # The plan is CHECKED against every batch (round 6): the residual / projection epilogues keep running maxima of exactly the two quantities
    # above (esme.attention.HalfGuard), `check_plan()` compares them with the plan at a synchronisation point -- predict_log_prob / predict_prob
    # do (and re-run the batch once with the widened plan when it was stale), esme.pipeline.StreamedInference does with each result -- and
    # `model(...)` stays asynchronous: call check_plan() yourself.  ESME_HALF_GUARD=0 switches the bookkeeping off.
    half_guard = os.environ.get('ESME_HALF_GUARD', '1') != '0'
    half_qp = os.environ.get('ESME_HALF_QP', '1') != '0'       # (A/B switch of HalfPlan.qp; read here only)
    half_check = 'sync'            # 'sync': predict_* check overflow + plan inline (one device synchronisation per call); 'defer': they do not -- the
                                   # caller polls check_overflow() / check_plan() (graph replays, latency-sensitive loops)
    HALF_CALIB_VOCAB = 'all'       # calibration tokens: 'all' = every id of the alphabet (specials, X B U Z O . -, <mask>); 'residues' = ids 4..23 + cls / eos (round 5)

    def set_precision(self, mode: str, robust=None, calib=None):
        """'fast' (default), 'high' (fp32 residual stream), 'half' (fp16 MFMA operands, fp16-pair residual stream: ~4e-4 of the fp32
        forward, fp32 outputs, ~1.1x the time) or 'exact' (split bf16 operand pairs: the reference's fp32 forward to ~1e-5, fp32 outputs,
        ~2.2x the time); DESIGN.md section 4 has what each achieves.  `robust` ('half' only): 'auto' (default; see `half_robust`), True,
        False, or a ready esme.attention.HalfPlan.  `calib` ('half' only): `(tokens, cu_lens)` or `(tokens, (cu_lens, max_len))` of the caller's
        OWN data, packed like a forward's input -- calibrated on in addition to the built-in whole-vocabulary batch (the plan is then decided
        on what the model will really see; the run-time guard covers the rest)."""
        assert mode in ('fast', 'high', 'half', 'exact'), mode
        if self.has_lora:
            lora_fused.check_precision(mode)
        changed = mode != self.precision
        self.precision = mode
        if halfmode.configure(self, robust, calib) or changed:
            self._drop_derived()                              # (keeps the plan just decided on; invalidate_graphs() would recalibrate)
        return self

    def half_plan(self, device=None):
        """The HalfPlan precision 'half' runs with on this model (calibrated on first use; see `half_robust`)."""
        return halfmode.half_plan(self, device)

    @property
    def _half_guard(self):
        """The HalfGuard of precision 'half' (read-only; None before the first 'half' forward or with half_guard off): `half_mode.guard`."""
        return self.half_mode.guard

    def check_plan(self, update: bool = True):
        """Compare what the forwards in precision 'half' since the last call actually saw with what the plan assumed: a stream channel outside the
        extension tile whose largest |value| exceeds HALF_CHANNEL_RATIO x the median channel's, or a layer without q / k pairs whose score bound
        reaches HALF_SCORE_BOUND, means the 1e-3 of the mode no longer rests on a measurement ("plan stale").  Synchronises with the device; the
        maxima are cleared.  Returns None when the plan held, else a dict {'channels': [(id, ratio), ...], 'layers': [(layer, bound), ...],
        'updated': bool, 'message': str}.  `update=True` widens the plan in place (the offending channels join the extension tile, up to 64; the
        offending layers get q / k pairs where the block has that form), so that the NEXT forward is covered -- re-run the batch that tripped it
        (predict_log_prob / predict_prob do that themselves).  A RuntimeWarning accompanies every stale verdict.  Coverage: the channel check runs
        in every residual epilogue of every model; the score check in the LayerNorm-folded projections with fused rotary (ESM-2 family, head
        dims 16 / 32 / 64) and in ESM-C's q / k LayerNorm + rotary pass -- ESM-1b / 1v (no rotary) and head dim 128 rely on the calibration for it.
        The maxima carry the unit of q they were recorded in (HalfGuard.q_scaled: the projection records q after the fixed-reference form's
        q scale, ESM-C's pass before it) and are converted when a plan of the other unit runs, so a plan change between the forwards and this
        check reads the same bound.  A verdict no plan can cover (more than 64 massive channels; large scores in a block without a q/k-pair
        form) returns 'updated': False, 'uncovered': True and changes nothing -- no new plan, no new descriptor or graph, no re-run in
        predict_* -- and warns once per plan.  After editing weights in place, invalidate_graphs() drops the plan: the next forward recalibrates."""
        vec = halfmode.guard_snapshot(self)
        return None if vec is None else halfmode.plan_verdict(self, vec.cpu(), update)              # the one synchronisation

    def _apply(self, fn, *a, **kw):
        """`.to()`, `.cuda()`, dtype casts: the parameters' storage moves -- drop everything derived from it."""
        out = super()._apply(fn, *a, **kw)
        self.invalidate_graphs()              # (drops the plan too: its channel list lives on the old device; recalibrated on first use)
        return out

    def load_state_dict(self, *a, **kw):
        out = super().load_state_dict(*a, **kw)
        self.invalidate_graphs()              # (drops the plan too: other weights, other plan)
        return out

    # -- helpers ---------------------------------------------------------------
    def _context(self, cu_lens, max_len, total, device) -> ForwardContext:
        pos, _ = _hip.seq_positions(cu_lens, total)
        rot = self.layers[0].self_attn.rot_emb if len(self.layers) else None
        cos = sin = None
        st = self.half_mode
        plan, ovf, guard = st.for_forward(self, device) if self.precision == 'half' else (None, None, None)
        cos32 = sin32 = None
        if rot is not None:
            dt = {'exact': torch.float32, 'half': torch.float16}.get(self.precision, torch.bfloat16)
            if plan is not None and plan.qk_pair:                 # q / k pairs are rotated with fp32 tables (in the projection's pair epilogue),
                cos32, sin32 = rot.tables(int(max_len), device, torch.float32)      # the other layers with the mode's fp16 tables
            cos, sin = rot.tables(int(max_len), device, dt)
        return ForwardContext(pos, cos, sin, fold=self.fold_layernorm, exact_attn=self.precision == 'high', f16=self.precision == 'half',
                              plan=plan, cos32=cos32, sin32=sin32, probe=st.probe, ovf=ovf, guard=guard)

    def check_overflow(self):
        """Raise OverflowError if a forward in precision 'half' since the last call saw a value leave IEEE fp16's range (|x| >= 65 504 in the
        residual stream, q / k / v or the FFN intermediate: it becomes inf, the result NaN).  Synchronises with the device; the flag is
        cleared.  predict_log_prob / predict_prob call it (their result is about to be read anyway); `model(...)` / `forward_representation`
        do not synchronise -- call it yourself before trusting their output, or read NaNs.  The bf16 modes ('fast', 'high', 'exact') have
        bf16's range (= fp32's) and nothing to check."""
        return halfmode.check_overflow(self)

    def _unpad(self, x, tokens):
        """Boolean-mask row gather: the `unpad_input` contract (esm.py:238)."""
        indices, cu_lens, max_len = self._unpad_index(tokens)
        return _hip.gather_rows(x.view(-1, x.shape[-1]), indices), indices, cu_lens, max_len

    def _unpad_index(self, tokens):
        """(flat indices of the rows that are not `<pad>`, cu_lens, max_len) of 2-D tokens."""
        keep = tokens.ne(self.alphabet.padding_idx)
        lens = keep.sum(dim=1, dtype=torch.int32)
        indices = torch.nonzero(keep.flatten(), as_tuple=False).flatten()
        cu_lens = torch.zeros(tokens.shape[0] + 1, dtype=torch.int32, device=tokens.device)
        cu_lens[1:] = torch.cumsum(lens, 0)
        return indices, cu_lens, int(lens.max())

    @staticmethod
    def _pad(x, indices, batch, seqlen):
        """`pad_input`: scatter packed rows into zeros (B*S, E) -> (B, S, E) (esm.py:255).  fp32 rows (precision 'exact') move as
        twice as many 16-bit words: the kernel copies 16-byte chunks."""
        if x.dtype == torch.float32:
            y = _hip.scatter_rows(x.contiguous().view(torch.bfloat16), indices, batch * seqlen)
            return y.view(torch.float32).view(batch, seqlen, x.shape[-1])
        return _hip.scatter_rows(x, indices, batch * seqlen).view(batch, seqlen, x.shape[-1])

    def _check_layers_arg(self, layers):
        assert all(i < len(self.layers) for i in layers), \
            f'Invalid layer indices {layers}. The number of layers in the model is {len(self.layers)}.'

    # -- forward -----------------------------------------------------------------
    def forward_representation(self, tokens, pad_args=None, pad_output=False, pad_indices=None,
                               lora_names=None, layers=None):
        """Per-token representations: (T, E) for packed input, (B, S, E) when padded;
        with `layers=[...]` the raw outputs of those layers are concatenated after the
        final-LayerNorm output on the feature axis (esm.py:201-266).  `lora_names`: the adapters to apply on a model that has
        some (None / empty: all of them; an unknown name raises KeyError)."""
        layers = list(layers) if layers else []
        self._check_layers_arg(layers)

        with _hip.stream_scope(self.embed_tokens.weight.device):
            x = self._forward_representation(tokens, pad_args, pad_output, pad_indices, layers, lora_names=lora_names)
            if self.padded:                                       # physical -> logical width, per concatenated block
                E, Ep = self.embed_dim, self.phys_dim
                x = torch.cat([x[..., i * Ep:i * Ep + E] for i in range(x.shape[-1] // Ep)], dim=-1)
            return x

    def _forward_representation(self, tokens, pad_args, pad_output, pad_indices, layers, want_pair=False, lora_names=None, observer=None):
        """forward_representation at the PHYSICAL width (== the logical one unless the layout is padded).  `want_pair`
        (precision 'exact' only): return the (hi, lo) bf16 pair of the final-LayerNorm output, the LM head's operand.
        `observer` (_observe, precision 'fast'): called with (cu_lens, max_len), returns the esme.qk_observer.QKObserver that every
        attention block hands its (q, k) to; the layers then run through the per-layer module loop, as with `layers=[...]`."""
        lora = self._lora_select(lora_names)                   # None without adapters; else the names this call applies
        x = self._embedding_phys(tokens, pad_args)
        if pad_args is not None:
            assert tokens.ndim == 1, 'tokens are expected to be unpadded with shape (batch * seq_len)'
            cu_lens, max_len = pad_args
        else:
            assert tokens.ndim == 2, 'tokens are expected to be padded with shape (batch, seq_len, embed_dim)'
            x, pad_indices, cu_lens, max_len = self._unpad(x, tokens)
        if cu_lens.dtype != torch.int32:
            cu_lens = cu_lens.to(torch.int32)
        max_len = int(max_len)

        # width the 2-D path pads back to: the INPUT width.  unpad_input's indices live on the (B, S) input grid;
        # the reference pads to max(lens) (esm.py:255), which equals S for every input it accepts (with S > max(lens)
        # its pad_input raises an index error) -- using S keeps the scatter in bounds for fixed-width batches too.
        pad_width = tokens.shape[1] if pad_args is None else max_len
        ctx = self._context(cu_lens, max_len, x.shape[0], x.device)
        if observer is not None:
            ctx.observer = observer(cu_lens, max_len)
        # one mode, one method: (final-LayerNorm output, raw outputs of the layers in `layers`).  'high' without layers is the fast path.
        mode = self.precision if self.precision in ('half', 'exact') or (self.precision == 'high' and len(self.layers)) else 'fast'
        x, taps = getattr(self, '_run_' + mode)(x, (tokens, pad_args, pad_indices), cu_lens, max_len, ctx, layers, want_pair, lora)
        return self._finish_representation(x, taps, pad_output, pad_args, pad_indices, cu_lens, pad_width)

    def _one_call(self, ctx, layers, mode) -> bool:
        """May this forward take the one-call C entry of `mode` (esme.cforward)?  Not with `layers=[...]` taps, a (q, k) observer or an
        active launch trace: those need the per-layer module loop."""
        return bool(self.c_forward and not layers and ctx.observer is None and _hip.TRACE is None and self._c_forward_ok(mode))

    def _final_pair(self, T, device, pair=None):
        """'exact' / 'half': the final LayerNorm's (hi, lo) bf16 pair (or the one given) and its fp32 output."""
        alloc = torch.zeros if self.padded else torch.empty
        Ep = self.phys_dim
        return pair if pair is not None else alloc(T, 2 * Ep, dtype=torch.bfloat16, device=device), alloc(T, Ep, dtype=torch.float32, device=device)

    def _run_fast(self, x, embed_args, cu_lens, max_len, ctx, layers, want_pair, lora):
        if self._one_call(ctx, layers, 'fast'):
            from esme import cforward
            return cforward.forward_layers(self, x, cu_lens, max_len, ctx.pos, ctx.cos, ctx.sin), []
        taps, E = [], self.embed_dim
        ctx.order = _hip.seq_order(cu_lens)     # longest sequences' attention work first (speed only; the C entry does the same)
        if lora is not None:
            x = self._lora_stream(x, lora, ctx)
        for i, layer in enumerate(self.layers):
            x = layer(x, cu_lens, max_len, lora, ctx, inplace=True)
            if i in layers:
                taps.append(x.clone(memory_format=torch.contiguous_format) if lora is not None else x.clone())
        if ctx.lora_x is not None:                                # the stream lives inside the wide buffer: the final LayerNorm moves it out
            y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
            self.emb_layer_norm_after(x, out=y)
            return y, taps
        self.emb_layer_norm_after(x[:, :E], out=x[:, :E])        # pad columns (if any) stay zero
        return x, taps

    def _run_high(self, x, embed_args, cu_lens, max_len, ctx, layers, want_pair, lora):
        """fp32 residual stream; x (bf16) is kept as the rounded copy the GEMMs read."""
        assert x.shape[1] % 64 == 0, 'high-precision mode needs a 64-aligned physical width'
        taps, E = [], self.embed_dim
        ctx.fp32_stream(torch.empty(x.shape, dtype=torch.float32, device=x.device), x, len(self.layers))
        ctx.sums = torch.empty(1, x.shape[0], 2, dtype=torch.float32, device=x.device)
        _hip.residual_f32_(ctx.x32, x, 1.0, x, ctx.sums, init=True)
        for i, layer in enumerate(self.layers):
            layer.forward_high_precision(x, cu_lens, max_len, ctx)
            if i in layers:
                taps.append(x.clone())
        ln = self.emb_layer_norm_after
        _hip.layernorm_f32(ctx.x32[:, :E], ln.weight, ln.bias, ln.eps, out=x[:, :E])
        return x, taps

    def _run_half(self, x, embed_args, cu_lens, max_len, ctx, layers, want_pair, lora):
        """fp16 MFMA operands: hi of the pair stream is what the LayerNorm-folded GEMMs read; the final LayerNorm and the LM head run in
        the split-operand form (fp32 representation / logits)."""
        (T, Ep), dev = x.shape, x.device
        x32 = self._embedding_exact(x, *embed_args)
        if self._one_call(ctx, layers, 'half'):
            # all layers + the final LayerNorm through ONE C call (esme_hip_forward_half: the launches below, bit-identical)
            from esme.cforward import forward_layers_half
            pair, rep32 = self._final_pair(T, dev)
            forward_layers_half(self, x32, cu_lens, max_len, ctx.pos, ctx.cos, ctx.sin, pair, rep32, ctx.plan, ctx.ovf, ctx.cos32, ctx.sin32, ctx.guard)
            return (pair if want_pair else rep32), []
        # the stream as a float16 PAIR [hi | lo] (x = hi + lo: 22 significant bits): hi is the operand of the LayerNorm-folded GEMMs,
        # the residual GEMMs read and write the pair in place (8 B per element in whole lines; an fp32 stream + operand copy is 10).
        # Padded layouts (ESM2-35M): everything at the physical width, pad columns zero as in the fast mode.
        # With massive channels (ctx.plan.ext_sel) the row is [hi | ext (64) | lo]: the LayerNorm-folded GEMMs read [hi | ext] (K = Ep + 64).
        taps, ext = [], ctx.plan.ext
        # (stored scaled per column by rho of the LayerNorm that reads it next: attention._fold_layernorm_pow2)
        scales = [(layer.self_attn.stream_scale(), layer.stream_scale()) for layer in self.layers]
        ctx.pair_stream(torch.empty(T, 2 * Ep + ext, dtype=torch.float16, device=dev), scales)
        ctx.sums = torch.empty(1, T, 2, dtype=torch.float32, device=dev)
        _hip.stream_operand(x32, ctx.xs, ctx.sums, pair=True, scale=scales[0][0][0], ext_sel=ctx.plan.ext_sel,
                            col_absmax=ctx.guard.col[0] if ctx.guard is not None else None)
        del x32
        x16 = ctx.xs[:, :Ep + ext]
        ctx.order = _hip.seq_order(cu_lens)
        last = len(self.layers) - 1
        for i, layer in enumerate(self.layers):
            layer.forward_high_precision(x16, cu_lens, max_len, ctx)
            if i in layers:
                tap = _hip.pair_to_f32(ctx.xs, Ep)
                taps.append(tap * scales[i + 1][0][1] if i < last else tap)          # the raw layer output: undo the stream's column scaling
        ln = self.emb_layer_norm_after
        pair, rep32 = self._final_pair(T, dev)
        _hip.layernorm_split(ctx.xs, ln.weight, ln.bias, ln.eps, self.embed_dim, out=pair, out32=rep32, in_off=Ep + ext, out_off=Ep, overflow_flag=ctx.ovf)
        return (pair, []) if want_pair else (rep32, taps)

    def _run_exact(self, x, embed_args, cu_lens, max_len, ctx, layers, want_pair, lora):
        """split-operand mode: fp32 residual stream, activation pairs, fp32 results (esme.attention.FlashTransformerLayer.forward_exact).
        Padded layouts (ESM2-35M): everything at the physical width, pad columns zero as in the other modes."""
        (T, Ep), dev = x.shape, x.device
        ctx.x32 = self._embedding_exact(x, *embed_args)
        if self._one_call(ctx, layers, 'exact'):
            # all layers + the final LayerNorm through ONE C call (esme_hip_forward_exact: the launches below, bit-identical)
            from esme.cforward import forward_layers_exact
            pair, rep32 = self._final_pair(T, dev)
            forward_layers_exact(self, ctx.x32, cu_lens, max_len, ctx.pos, ctx.cos, ctx.sin, pair, rep32)
            return (pair if want_pair else rep32), []
        taps = []
        ctx.order = _hip.seq_order(cu_lens)
        for i, layer in enumerate(self.layers):
            layer.forward_exact(cu_lens, max_len, ctx)
            if i in layers:
                taps.append(ctx.x32.clone())
        ln = self.emb_layer_norm_after
        pair, rep32 = self._final_pair(T, dev, ctx.scratch.get('h'))
        _hip.layernorm_split(ctx.x32, ln.weight, ln.bias, ln.eps, self.embed_dim, out=pair, out32=rep32, out_off=Ep)
        return (pair, []) if want_pair else (rep32, taps)

    def _finish_representation(self, x, taps, pad_output, pad_args, pad_indices, cu_lens, pad_width):
        if pad_output or (pad_args is None):
            nseq = cu_lens.numel() - 1
            x = self._pad(x, pad_indices, nseq, pad_width)
            taps = [self._pad(t, pad_indices, nseq, pad_width) for t in taps]
        return torch.concat((x, *taps), dim=-1) if taps else x

    def forward(self, tokens, pad_args=None, pad_output=False, pad_indices=None, lora_names=None):
        """Logits (T, V) / (B, S, V), bf16 (fp32 with precision 'exact' / 'half'), on the model's device (esm.py:268-282)."""
        with _hip.stream_scope(self.embed_tokens.weight.device):
            if self.precision in ('exact', 'half'):           # fp32 logits from the (hi, lo) pair of the final LayerNorm
                pair = self._forward_representation(tokens, pad_args, pad_output, pad_indices, [], want_pair=True, lora_names=lora_names)
                y = self.lm_head.forward_exact(pair.reshape(-1, pair.shape[-1]))
                return y.view(*pair.shape[:-1], y.shape[-1])
            return self.lm_head(self._forward_representation(tokens, pad_args, pad_output, pad_indices, [], lora_names=lora_names))

    def predict_log_prob(self, tokens, pad_args=None, pad_output=False, pad_indices=None, lora_names=None):
        with _hip.stream_scope(self.embed_tokens.weight.device):
            return halfmode.checked_run(self, lambda: _hip.softmax_rows(self(tokens, pad_args, pad_output, pad_indices, lora_names), log=True), tokens)

    def predict_prob(self, tokens, log=False, pad_args=None, pad_output=False, pad_indices=None,
                     lora_names=None):
        with _hip.stream_scope(self.embed_tokens.weight.device):
            return halfmode.checked_run(self, lambda: _hip.softmax_rows(self(tokens, pad_args, pad_output, pad_indices, lora_names), log=bool(log)), tokens)

    # -- contact prediction (esme/contacts.py) -----------------------------------------
    def set_contact_head(self, head):
        """Install the contact regression: a ContactHead, or anything ContactHead.load accepts (a safetensors / torch file, a state
        dict).  ValueError unless it has num_layers * attention_heads features.  ESM-C and adapted or fine-tuned models ship no contact
        regression: fit one on proteins of known structure with esme.fit_contact_head(model, batches, contact_maps) (contact_features + ContactHead.fit)."""
        from esme.contacts import ContactHead
        L, H = len(self.layers), self.attention_heads
        if not isinstance(head, ContactHead):
            head = ContactHead.load(head)
        n = head.regression.weight.numel()
        if n != L * H:
            raise ValueError(f'contact head with {n} features does not fit a model with {L} layers x {H} heads = {L * H}')
        if (head.num_layers, head.attention_heads) != (L, H):
            fitted = ContactHead(L, H, head.prepend_bos, head.append_eos)
            fitted.regression.weight.data.copy_(head.regression.weight.data.reshape(1, -1))
            fitted.regression.bias.data.copy_(head.regression.bias.data.reshape(1))
            head = fitted
        self.contact_head = head.to(device=self.embed_tokens.weight.device, dtype=torch.float32)
        return self

    def predict_contacts(self, tokens, pad_args=None, pad_output=False, logits=False, lora_names=None, _keep_qk=False):
        """Contact probabilities (`logits=True`: the logits) between the residues of every protein, float32.  Packed input
        (`pad_args=(cu_lens, max_len)`): a list of B (n_s, n_s) views of one buffer, n_s = the sequence's length without bos / eos; 2-D
        tokens or `pad_output=True`: (B, S - f - e, S - f - e) with zeros outside each protein's block.  Runs the forward in precision
        'fast' with one extra kernel call per layer (esme_hip_contact_layer); no attention map is stored."""
        if self.contact_head is None:
            raise RuntimeError('predict_contacts: the model has no contact head (model.set_contact_head(head or path); ESM-C ships none)')
        from esme.contacts import ContactAccumulator
        head = self.contact_head
        acc = self._observe('predict_contacts', tokens, pad_args, lora_names, _keep_qk,
                            lambda cu_lens, max_len, *hd: ContactAccumulator(head, cu_lens, max_len, *hd, keep_qk=_keep_qk))
        maps = acc.result(len(self.layers), logits)
        if not (pad_output or pad_args is None):
            return maps
        width = (tokens.shape[1] if pad_args is None else acc.max_len) - sum(head.trim)
        return dense_blocks(maps, (), width, torch.float32, acc.out.device)

    def _observe(self, what, tokens, pad_args, lora_names, keep_qk, make):
        """The packed forward of `what` (predict_contacts / contact_features / attention_maps) with a (q, k) observer installed:
        `make(cu_lens, max_len, heads, head_pad, head_dim)` builds it once the batch's geometry is known, every attention block hands
        it its final (q, k), and it is returned.  `keep_qk` (tests): its `.qk` is left in `self._contact_qk`."""
        if self.precision != 'fast':
            raise NotImplementedError(f"{what} runs in precision 'fast' only; precision {self.precision!r} is not implemented "
                                      "(set_precision('fast'))")
        box = []

        def observer(cu_lens, max_len):
            box.append(make(cu_lens, max_len, self.attention_heads, self.head_pad, self.embed_dim // self.attention_heads))
            return box[0]
        with _hip.stream_scope(self.embed_tokens.weight.device):
            self._forward_representation(tokens, pad_args, False, None, [], lora_names=lora_names, observer=observer)
        if keep_qk:
            self._contact_qk = box[0].qk
        return box[0]

    def contact_features(self, tokens, pad_args=None, pairs=None, min_sep=0, lora_names=None, _keep_qk=False):
        """The contact regression's features at residue pairs: (X, pairs), X float32 (P, num_layers * attention_heads) on the device with
        X[p, l * H + h] = N^(l,h)_ij (the symmetrised, APC-corrected attention of layer l, head h; esme/contacts.py), pairs int32 (P, 3)
        rows (s, i, j) with i, j counting the residues of sequence s without bos / eos.  pairs=None: every i < j with j - i >= min_sep
        of every sequence (min_sep is not applied to a list you pass); else an integer (P, 3) tensor, or a list of one (P_s, 2)
        tensor of (i, j) rows per sequence -- ValueError on a row out of range.  Needs no contact head: this is what
        ContactHead.fit is trained on.  Runs the forward in precision 'fast' with one extra kernel call per layer
        (esme_hip_contact_features); no attention map is stored."""
        from esme.contacts import ContactFeatureAccumulator, all_pairs, check_pairs

        def make(cu_lens, max_len, *hd):
            n = (cu_lens[1:] - cu_lens[:-1] - 2).clamp(min=0).tolist()          # the alphabets put one bos and one eos around every protein
            rows = all_pairs(n, min_sep, cu_lens.device) if pairs is None else check_pairs(pairs, n, cu_lens.device)
            return ContactFeatureAccumulator(rows, cu_lens, max_len, len(self.layers), *hd, trim=(1, 1), keep_qk=_keep_qk)
        acc = self._observe('contact_features', tokens, pad_args, lora_names, _keep_qk, make)
        return acc.result(len(self.layers)), acc.pairs

    # -- attention maps (esme/attention_maps.py) -----------------------------------------
    def attention_maps(self, tokens, pad_args=None, pad_output=False, layers=None, heads=None, head_weights=None,
                       dtype=torch.float32, lora_names=None, max_bytes=4 << 30, _keep_qk=False):
        """Attention weights softmax(q k^T * scale) of chosen layers and heads, bos / eos rows and columns included (what fair-esm's
        need_head_weights=True and Hugging Face's output_attentions=True return).  `layers` / `heads`: index lists (negative indices count
        from the end, None = all; IndexError out of range, ValueError on duplicates).  `head_weights`: None, 'mean' (1 / number of
        selected heads) or a float tensor (len(layers), len(heads)): the selected heads of each layer are summed with these weights into
        ONE map per layer.  `dtype`: torch.float32 or torch.bfloat16.  Packed input (`pad_args=(cu_lens, max_len)`): a list of B views
        of one buffer, each (L_sel, H_sel, S_b, S_b) -- with head_weights (L_sel, S_b, S_b); 2-D tokens or `pad_output=True`: a dense
        (B, L_sel, H_sel, S, S) / (B, L_sel, S, S) tensor, zero outside each protein's block.  The buffer takes
        L_sel * n_out * sum_b S_b^2 * itemsize bytes (n_out = H_sel, or 1 with head_weights): ValueError before the forward runs when
        that exceeds `max_bytes`.  Runs the forward in precision 'fast' with one extra kernel call per SELECTED layer
        (esme_hip_attn_maps)."""
        from esme import attention_maps as AM
        if dtype not in AM.DTYPES:
            raise ValueError(f'attention_maps: dtype must be torch.float32 or torch.bfloat16, got {dtype}')
        lsel = AM.select_indices(layers, len(self.layers), 'layers')
        hsel = AM.select_indices(heads, self.attention_heads, 'heads')
        weights = AM.check_head_weights(head_weights, len(lsel), len(hsel))
        n_out = 1 if weights is not None else len(hsel)
        if pad_args is not None:
            lengths = (pad_args[0][1:] - pad_args[0][:-1]).tolist()
        else:
            lengths = tokens.ne(self.alphabet.padding_idx).sum(dim=1).tolist()
        need = AM.buffer_bytes(lengths, len(lsel), n_out, dtype)
        if need > max_bytes:
            raise ValueError(f'attention_maps: the maps need {need} bytes (L_sel * n_out * sum_b S_b^2 * itemsize = {len(lsel)} * {n_out} * '
                             f'{sum(s * s for s in lengths)} * {2 if dtype == torch.bfloat16 else 4}), more than '
                             f'max_bytes = {max_bytes}: select fewer layers= or heads=, pass head_weights= (one map per layer), use '
                             'dtype=torch.bfloat16, send fewer or shorter proteins per call, or raise max_bytes=')
        acc = self._observe('attention_maps', tokens, pad_args, lora_names, _keep_qk,
                            lambda *geometry: AM.AttentionMapAccumulator(lsel, hsel, weights, dtype, *geometry, keep_qk=_keep_qk))
        maps = acc.result()
        if not (pad_output or pad_args is None):
            return maps
        lead = (len(lsel),) if weights is not None else (len(lsel), n_out)
        return dense_blocks(maps, lead, tokens.shape[1] if pad_args is None else acc.max_len, dtype, acc.out.device)

    def graphed(self, tokens, pad_args, what: str = 'forward', clone: bool = True):
        """`getattr(self, what)(tokens, pad_args)` replayed from a hipGraph captured on first use of this
        input shape (esme/graph.py).  For repeated shapes of small batches, where ~160 Python-issued launches
        cost more than the GPU work.  With `clone=False` the result is a static buffer that the next replay of
        the same shape overwrites.  'predict_log_prob' in precision 'half' with half_check = 'sync' checks the token ids, the range flag and the
        plan after each replay, as the eager call does (a widened plan is re-captured and replayed once)."""
        if what in ('predict_contacts', 'contact_features', 'attention_maps'):
            raise NotImplementedError(f'graphed(): hipGraph replay of {what} is not implemented; call model.{what} directly')
        assert what in ('forward', 'forward_representation', 'predict_log_prob')
        if self.has_lora:
            raise NotImplementedError('graphed(): hipGraph replay is not implemented for a model with LoRA adapters (a graph bakes one adapter '
                                      'selection and its derived weights in); call the model directly')
        if getattr(self, '_graph_cache', None) is None:
            from esme.graph import GraphCache
            self._graph_cache = GraphCache(self)

        def replay():                                      # (a capture warms up with the checks deferred: esme.graph)
            return self._graph_cache.run(what, tokens, pad_args, clone)
        # (as eager predict_log_prob does, once after the replay: it sets the same sticky flags; a widened plan dropped the captured graphs, so the re-run captures anew)
        return halfmode.checked_run(self, replay, tokens, recheck=False) if what == 'predict_log_prob' else replay()

    def invalidate_graphs(self):
        """Forget captured hipGraphs, the C-entry model descriptor AND the calibrated HalfPlan of precision 'half' -- call it after changing
        weights in place, in particular through `p.data`, which bumps no version counter: the next 'half' forward recalibrates on the
        edited weights (a plan decided on the old ones would keep their massive channels and score bounds), and every derived weight copy
        (LN-folded, fp16, extension-tile, packed, padded) is rebuilt from them on next use."""
        self.half_mode.plan = None
        bump_weights_epoch()                  # every derived weight copy is rebuilt on next use (its key holds the epoch: esme.nn.version_key)
        self._drop_derived()

    def _drop_derived(self):
        """invalidate_graphs() without the plan: what set_precision / a widening plan verdict call after installing the plan they decided on."""
        if getattr(self, '_graph_cache', None) is not None:
            self._graph_cache.clear()
        self.__dict__.pop('_cdesc', None)
        self.__dict__.pop('_cdesc16', None)
        self.__dict__.pop('_cdesc_exact', None)
        self.__dict__.pop('_cparams', None)
        self.__dict__.pop('_cws', None)
        bump_epoch()

    # -- LoRA adapters (inference; esme/lora.py) ---------------------------------------------------------------------
    _LORA_TARGETS = (('query', 'q'), ('key', 'k'), ('value', 'v'), ('output', 'out'))
    _LORA_FFN_TARGETS = ('ffn_up', 'ffn_down')       # the layer's FFN projections (FlashTransformerLayer.wrap_ffn_lora)

    @property
    def has_lora(self) -> bool:
        return bool(self.__dict__.get('_lora_attached', False))

    def _lora_select(self, lora_names):
        """None on a model without adapters (`lora_names` is then ignored, as in the reference); else the tuple of adapter names this call
        applies -- all of them for None / an empty list.  KeyError for an unknown name; NotImplementedError where the adapters could not
        be applied (any precision but 'fast', train mode): a forward never runs silently without them."""
        if not self.has_lora:
            return None
        lora_fused.check_precision(self.precision)
        lora_fused.check_mode(self.training)
        have = self.lora_names()
        if not lora_names:
            return tuple(have)
        for n in lora_names:
            if n not in have:
                raise KeyError(f'LoRA adapter {n!r} not found (available: {have})')
        return tuple(lora_names)

    def lora_names(self) -> list:
        """Names of the attached adapters, in the order they were added."""
        from esme.lora import lora_modules
        mods = lora_modules(self)
        return list(mods[0].lora_A.keys()) if mods else []

    def _lora_stream(self, x, lora, ctx):
        """The residual stream moved into the first E columns of a (T, E + X) buffer (X: the wider of the extension K-tiles of the QKV GEMM
        and of the FFN up-projection for this adapter selection): every layer's esme_hip_lora_down writes next to the stream, and the
        LayerNorm-folded QKV / FFN-up GEMM reads [x | u] as ONE operand.  Returns the stream as a view of that buffer (x itself when
        neither GEMM carries an adapter)."""
        X = max(self.layers[0].self_attn.lora_ext_widths(lora)[0], self.layers[0].ffn_lora_ext_widths(lora)[0])
        if not X or not ctx.fold or x.shape[1] % 64:
            return x
        T, E = x.shape
        ctx.lora_x = torch.empty(T, E + X, dtype=x.dtype, device=x.device)
        ctx.lora_x[:, :E].copy_(x)                                # (row move, no arithmetic)
        return ctx.lora_x[:, :E]

    def add_lora(self, rank=16, alpha=16, layers=('query', 'value', 'output'), dropout_p=0., adapter_names=None, quantized_base=False):
        """Attach LoRA adapters (reference esm.py:495-543): every layer's `self_attn.{q,k,v,out}` named in `layers` becomes an
        esme.lora.LoRA around the projection, with one (A, B) pair per name in `adapter_names` (default ['default']).  Beyond the
        reference's four names, 'ffn_up' wraps the FFN up-projection (`final[1]` of a GELU layer; SwiGLU's `final[1].activation` and
        `final[1].fc`, one adapter of that rank each) and 'ffn_down' the down-projection (`final[3]` / `final[2]`): with all six,
        every linear layer of the block carries an adapter (the QLoRA recipe).  A is initialised
        like the reference's (Kaiming uniform), B with zeros, so fresh adapters leave the model's output unchanged.  Inference only:
        `dropout_p` is stored (and written by save_lora) but never applied.  Refuses what cannot run the adapters: a precision other
        than 'fast', quantised base weights, padded layouts (ESM2-35M), ranks outside 1 .. 64.
        `quantized_base=True` opts a model loaded with `quantization=` in (QLoRA; on an unquantised model it changes nothing): the
        adapters are attached around the 4-bit / int8 projections, `forward_trainable` trains them (and the LM head after
        mark_lmhead) with the base expanded from the codes in forward and backward (esme.autograd.QuantFrozenLinear), and the fused
        inference forward runs them with the extension block placed next to the expanded base per call.  The codes are not
        trainable and the LayerNorms stay frozen (mark_trainable / a LayerNorm that requires grad keep raising)."""
        from esme.lora import LoRA
        wanted = set(layers)
        assert len(wanted.difference({'query', 'value', 'key', 'output', *self._LORA_FFN_TARGETS})) == 0, \
            'layers must be a subset of {"query", "value", "key", "output", "ffn_up", "ffn_down"}'
        if self.has_lora:
            raise NotImplementedError('LoRA adapters are already attached to this model (a second set would wrap the first)')
        lora_fused.check_precision(self.precision)
        quantised = getattr(self, 'quantization', None) is not None
        if quantised and not quantized_base:
            raise NotImplementedError('LoRA adapters need unquantised bfloat16 base weights (quantization= is not supported with adapters; '
                                      'opt in to adapters over the quantised base with add_lora(quantized_base=True))')
        if self.padded:
            raise NotImplementedError('LoRA adapters are not implemented for padded layouts (head dim 24 / a width that is not a multiple of 64: ESM2-35M)')
        if not (1 <= int(rank) <= 64) or int(rank) != rank:
            raise NotImplementedError(f'LoRA rank {rank}: integer ranks 1 .. 64 are served')
        self.lora_kwargs = {'rank': rank, 'alpha': alpha, 'dropout_p': dropout_p,
                            'layers': [long for long in (*(l for l, _ in self._LORA_TARGETS), *self._LORA_FFN_TARGETS) if long in wanted],
                            'names': adapter_names}

        def wrap(lin):
            return LoRA(lin, rank=rank, alpha=alpha, dropout_p=dropout_p, names=adapter_names)

        for layer in self.layers:
            att = layer.self_attn
            att.wrap_lora([short for long, short in self._LORA_TARGETS if long in wanted], wrap)
            layer.wrap_ffn_lora('ffn_up' in wanted, 'ffn_down' in wanted, wrap)
            att._qlora = layer._qlora = bool(quantised)      # (quantised here means: and opted in)
        self.__dict__['_lora_attached'] = True
        self._qlora = bool(quantised)
        self.mark_only_lora_as_trainable(adapter_names)
        self.invalidate_graphs()
        return self

    def mark_only_lora_as_trainable(self, adapter_names=None):
        from esme.lora import mark_only_lora_as_trainable
        mark_only_lora_as_trainable(self, adapter_names)
        return self

    def lora_state_dict(self, adapter_names=None):
        from esme.lora import lora_state_dict
        return lora_state_dict(self, adapter_names)

    def save_lora(self, path: str, adapter_names=None):
        """Write the adapters (all, or those named) to a safetensors file in the reference's format (esm.py:564-585): the
        `lora_A` / `lora_B` tensors under their state-dict keys, metadata rank / alpha / dropout_p / layers / names / format."""
        from safetensors.torch import save_file
        state = self.lora_state_dict(adapter_names)
        assert len(state) > 0, 'No LoRA adapters found to save'
        kw = self.lora_kwargs
        names = adapter_names or kw['names'] or self.lora_names()
        save_file({k: v.detach().contiguous() for k, v in state.items()}, path,
                  {'rank': str(kw['rank']), 'alpha': str(kw['alpha']), 'dropout_p': str(kw['dropout_p']),
                   'layers': ','.join(kw['layers']), 'names': ','.join(names), 'format': 'pt'})
        return self

    def load_lora(self, path: str, names=None, quantized_base=False):
        """Attach the adapters of a file written by `save_lora` (this package's or the reference's) to a model loaded from the base
        checkpoint (esm.py:587-608).  `names` is accepted for signature compatibility; as in the reference, every adapter of the file
        is attached -- select per call with `lora_names=`.  `quantized_base`: as in add_lora."""
        from safetensors import safe_open
        with safe_open(path, framework='pt', device='cpu') as f:
            md = f.metadata() or {}
            tensors = {k: f.get_tensor(k) for k in f.keys()}
        a = md['alpha']
        self.add_lora(rank=int(md['rank']), alpha=int(a) if a.lstrip('-').isdigit() else float(a), dropout_p=float(md['dropout_p']),
                      layers=md['layers'].split(','), adapter_names=md['names'].split(','), quantized_base=quantized_base)
        own = self.state_dict()
        unexpected = [k for k in tensors if k not in own]
        assert len(unexpected) == 0, f'Expected LoRA keys in the model missing state_dict: {unexpected}'
        missing = [k for k in self.lora_state_dict() if k not in tensors]
        assert len(missing) == 0, f'LoRA keys of the model missing in the file: {missing}'
        with torch.no_grad():
            for k, t in tensors.items():
                own[k].copy_(t)                                   # (bumps the version counter: derived weights are rebuilt)
        self.invalidate_graphs()
        return self

    # -- LoRA fine-tuning (esme/autograd.py) -------------------------------------------------------------------------
    def forward_trainable(self, tokens, pad_args=None, pad_output=False, pad_indices=None, lora_names=None, logits=True,
                          checkpoint_layers=False, layers=None):
        """model(...) with a grad_fn: logits (T, V) / (B, S, V), or with logits=False the final-LayerNorm representation, as a
        differentiable function of the adapters `lora_names` selects (None / empty: all), of the LM head where mark_lmhead(True)
        made it trainable, and of the layers' projections and LayerNorms where mark_trainable() did (full fine-tuning).  The
        reference's unfused data flow in bfloat16: the base projections (forward, dX and, where trained, dW / db) and the attention
        forward and backward are this package's kernels (esme.autograd.FrozenLinear / TrainableLinear / VarlenAttention), everything
        between them torch ops.  `checkpoint_layers=True` runs every layer under torch.utils.checkpoint (non-reentrant): only the
        layers' inputs are kept and each layer is recomputed in the backward -- the reference's `checkpointing=`; every kernel on the
        path is deterministic, so loss and gradients are bit-equal with and without it.  The same in train() and eval() (there is no
        dropout).  `model.train(); model(...)` still raises: the fused inference forward has no backward.  NotImplementedError, by
        name, for a precision other than 'fast', quantised weights (unless add_lora(quantized_base=True) opted in: then the adapters
        and the LM head train over the quantised base, and a LayerNorm that requires grad is refused), the padded ESM2-35M layout, dropout > 0, a head dim outside
        {32, 64}, the learned-position ESM-1 models without mark_trainable(positions=...) and a token embedding that requires grad
        without mark_trainable(embedding=True) (with it the table trains: esme.autograd.TokenEmbedding; quantised models stay refused).
        ESM-1b / ESM-1v after mark_trainable(positions=True or 'frozen'): the ids are packed, the lookup is
        esme.autograd.PositionEmbedding (the position table's gradient is esme_hip_embed_positions_bwd), ESM-1b's emb_layer_norm_before
        follows in torch ops, then the same layers; a max_len above the position table raises ValueError before any launch.
        `layers=[...]` (with logits=False; ValueError with logits=True, the LM head takes E columns) taps the raw outputs of those
        layers as forward_representation(layers=) does -- the same check of the indices, the same order (that of the model's layers)
        -- and concatenates them after the final-LayerNorm output on the feature axis: (T, (1 + k) E) / (B, S, (1 + k) E), every
        column block with a grad_fn, so that a head of width (1 + k) E trains the backbone through the taps (the reference's
        RegressionTrainer(layers=...)).  The taps are the tensors the next layer reads, not copies; None / empty changes nothing."""
        from esme import autograd as ag
        train_emb = bool(self.__dict__.get('_train_embedding', False))
        ag.refuse(self.embed_tokens.weight.requires_grad and not train_emb,
                  'embed_tokens.weight requires grad, but the token embedding has no backward: '
                  'select what to train with model.mark_trainable() (projections and LayerNorms), which leaves the embedding frozen')
        ag.refuse(self.precision != 'fast', f"precision {self.precision!r} has no backward: training runs in precision 'fast' only")
        qlora = bool(getattr(self, '_qlora', False))
        ag.refuse(getattr(self, 'quantization', None) is not None and not qlora,
                  f'quantised weights have no backward (load the model without quantization=; {ag.QLORA_HINT})')
        ag.check_frozen_norms((('emb_layer_norm_after', self.emb_layer_norm_after),), qlora)
        ag.refuse(self.padded, 'the padded layout (ESM2-35M: head dim 24, a width that is not a multiple of 64) has no backward')
        learned = type(self)._embedding_phys is not ESM2._embedding_phys
        train_pos = self.__dict__.get('_train_positions', False) if learned else False
        ag.refuse(learned and not train_pos, 'the learned-position models (ESM-1b / ESM-1v) are not covered')
        ag.refuse(learned and getattr(self, 'quantization', None) is not None,
                  'the learned-position models (ESM-1b / ESM-1v) do not train over quantised weights, with or without adapters')
        norm_before = getattr(self, 'emb_layer_norm_before', None) if learned else None
        if norm_before is not None:
            ag.check_frozen_norms((('emb_layer_norm_before', norm_before),), qlora)
        ag.refuse(train_emb and getattr(self, 'quantization', None) is not None,
                  'mark_trainable(embedding=True) on a quantised model: over a quantised base only the adapters and the LM head train')
        for layer in self.layers:
            layer.check_trainable()
        if self.has_lora and lora_names:
            have = self.lora_names()
            for n in lora_names:
                if n not in have:
                    raise KeyError(f'LoRA adapter {n!r} not found (available: {have})')
        names = tuple(lora_names) if lora_names else None
        tap_at = list(layers) if layers else []
        self._check_layers_arg(tap_at)
        if tap_at and logits:
            raise ValueError(f'forward_trainable: layers={tap_at} needs logits=False (the LM head takes the {self.embed_dim} columns of the '
                             'final-LayerNorm output, not the concatenation with the tapped layers)')
        taps = []
        with _hip.stream_scope(self.embed_tokens.weight.device):
            if pad_args is not None:
                assert tokens.ndim == 1, 'tokens are expected to be unpadded with shape (batch * seq_len)'
                cu_lens, max_len = pad_args
            else:
                assert tokens.ndim == 2, 'tokens are expected to be padded with shape (batch, seq_len, embed_dim)'
            if learned:
                # packed BEFORE the lookup, like the trainable token table below: the index of a kept row in the position table is its
                # in-sequence position + padding_idx + 1 for packed and for 2-D tokens (positions() counts the tokens that are no `<pad>`)
                pe = self.embed_positions
                limit = int(max_len) if pad_args is not None else tokens.shape[1]
                if limit > pe.max_positions:
                    raise ValueError(f'Sequence length {limit} above maximum  sequence length of {pe.max_positions}')
                if self.debug_checks:
                    self.check_tokens(tokens)
                if pad_args is None:
                    pad_indices, cu_lens, max_len = self._unpad_index(tokens)
                    tokens_packed = tokens.flatten()[pad_indices]
                else:
                    tokens_packed = tokens
                x = ag.PositionEmbedding.apply(self.embed_tokens.weight, pe.weight, tokens_packed, cu_lens, int(max_len),
                                               self.alphabet.mask_idx, pe.padding_idx + 1)
                if norm_before is not None:
                    x = ag.layer_norm(x, norm_before)
            elif train_emb:
                # the ids are packed BEFORE the lookup (the rows that are kept are the same rows): a `<pad>` row never reaches the
                # lookup, so it contributes nothing to the table's gradient, and 2-D tokens give the packed gradients
                if self.debug_checks:
                    self.check_tokens(tokens)
                if pad_args is None:
                    pad_indices, cu_lens, max_len = self._unpad_index(tokens)
                    tokens_packed = tokens.flatten()[pad_indices]
                else:
                    tokens_packed = tokens
                x = ag.TokenEmbedding.apply(self.embed_tokens.weight, tokens_packed, self.alphabet.mask_idx if self.zero_mask_rows else -1,
                                            self.alphabet.padding_idx if (pad_args is None and self.zero_mask_rows) else -1)
            else:
                x = self._embedding_phys(tokens, pad_args)
                if pad_args is None:
                    x, pad_indices, cu_lens, max_len = self._unpad(x, tokens)
            if cu_lens.dtype != torch.int32:
                cu_lens = cu_lens.to(torch.int32)
            max_len = int(max_len)
            pos, _ = _hip.seq_positions(cu_lens, x.shape[0])
            for i, layer in enumerate(self.layers):
                if checkpoint_layers:
                    from torch.utils.checkpoint import checkpoint
                    x = checkpoint(layer.forward_trainable, x, cu_lens, max_len, names, pos, use_reentrant=False)
                else:
                    x = layer.forward_trainable(x, cu_lens, max_len, names, pos)
                if i in tap_at:
                    taps.append(x)
            x = ag.layer_norm(x, self.emb_layer_norm_after)
            if pad_output or pad_args is None:                    # (before the head, as in forward(): pad rows hold head(0))
                width = tokens.shape[1] if pad_args is None else max_len
                x = ag.pad_rows(x, pad_indices, cu_lens.numel() - 1, width)
                taps = [ag.pad_rows(t, pad_indices, cu_lens.numel() - 1, width) for t in taps]
            if taps:
                return torch.cat((x, *taps), dim=-1)
            return self.lm_head.forward_trainable(x) if logits else x

    def masked_lm_loss(self, masked_tokens, pad_args, tokens, mask, lora_names=None, checkpoint_layers=False, reduction='mean'):
        """The masked-LM loss of a training step as a float32 device scalar with a grad_fn, without a host synchronisation: the
        sync-free form of `esme.cross_entropy(model.forward_trainable(masked_tokens, pad_args, ...), tokens, mask)`.
        forward_trainable(..., logits=False), then the LM head's dense -> GELU -> LayerNorm (RobertaLMHead.features_trainable, the ops
        of its forward_trainable), then the vocabulary projection fused with the cross-entropy (esme.autograd.LinearCrossEntropy on
        `lm_head.final`): the (T, V) logits are never formed, and the rows are selected by labels built on the device -- `tokens` where
        `mask` holds and the token is not `<pad>`, an ignored label elsewhere -- instead of a boolean index (a nonzero).  masked_tokens
        / tokens / mask: packed (T,) with pad_args = (cu_lens, max_len), or 2-D (B, S) with pad_args None.  The two routes agree to
        rounding but are not bit-equal: esme.cross_entropy reads logits that were rounded to bfloat16 first.  reduction: 'mean' (0,
        not NaN, when no row is selected) or 'sum'."""
        from esme.loss import linear_cross_entropy
        if tokens.shape != masked_tokens.shape or mask.shape != masked_tokens.shape:
            raise ValueError(f'masked_lm_loss: masked_tokens {tuple(masked_tokens.shape)}, tokens {tuple(tokens.shape)} and mask '
                             f'{tuple(mask.shape)} must have one shape')
        x = self.forward_trainable(masked_tokens, pad_args, lora_names=lora_names, logits=False, checkpoint_layers=checkpoint_layers)
        with _hip.stream_scope(self.embed_tokens.weight.device):
            h = self.lm_head.features_trainable(x)
            ignore = -100
            labels = torch.where(mask.to(torch.bool) & (tokens != self.alphabet.padding_idx), tokens, torch.full_like(tokens, ignore))
            return linear_cross_entropy(h, self.lm_head.final, labels.reshape(-1), ignore_index=ignore, reduction=reduction)

    def mark_lmhead(self, trainable=True):
        for p in self.lm_head.parameters():
            p.requires_grad_(trainable)
        return self

    # -- full fine-tuning (esme/autograd.py TrainableLinear, include/esme_hip_gemm_wgrad.h) --------------------------------------
    def mark_trainable(self, projections=True, norms=True, layers=None, embedding=False, positions=False):
        """Select what full fine-tuning trains through `forward_trainable`.  `projections`: requires_grad on the weights and biases of
        the selected layers' own projections (q, k, v, out, FFN up / down, SwiGLU's two; under a LoRA wrapper the base `layer`) --
        their gradients come from esme_hip_gemm_wgrad.  `norms`: on the selected layers' LayerNorms (ESM-C's q / k norms included) and,
        when `layers` is None, on `emb_layer_norm_after`, which belongs to no layer -- their gradients are torch's.  `layers`: indices
        (negative ones count from the end) for the "unfreeze the top k layers" recipe; None: all.  Every layer that is not selected
        is frozen, so `mark_trainable(False, False)` freezes the backbone again.  `embedding=True` opts the token embedding in
        (masked-LM training): requires_grad on `embed_tokens.weight`, and `forward_trainable` then runs the lookup as
        esme.autograd.TokenEmbedding, whose backward is esme_hip_embed_bwd.  `embedding=False` (the default) withdraws the opt-in, and
        clears the flag where the opt-in had set it; a flag set by hand is not touched, and `forward_trainable` keeps refusing it.  The
        LM head and LoRA adapters keep their flags (mark_lmhead, mark_only_lora_as_trainable).
        `positions` is the opt-in of the learned-position models (ESM-1b / ESM-1v), which `forward_trainable` refuses without it:
        True sets requires_grad on `embed_positions.weight` (its gradient is esme_hip_embed_positions_bwd; with
        `mark_trainable(False, False, positions=True)` the table trains alone, the run that made the 4 096-position checkpoints);
        'frozen' opts in and leaves the table frozen (LoRA, task-head or top-layer fine-tuning of these models); False (the default)
        withdraws the opt-in and clears a flag the opt-in had set.  With `norms` and `layers=None`, ESM-1b's `emb_layer_norm_before` is
        trained like `emb_layer_norm_after`.  ValueError for a truthy `positions` on a model without a position table."""
        from esme.lora import LoRA
        if embedding and getattr(self, 'quantization', None) is not None:
            raise NotImplementedError('mark_trainable(embedding=True): the token embedding does not train on a quantised model')
        if positions not in (False, True, 'frozen'):
            raise ValueError(f"mark_trainable: positions must be False, True or 'frozen', got {positions!r}")
        if positions != 'frozen':
            positions = bool(positions)
        pe = getattr(self, 'embed_positions', None)
        if positions and pe is None:
            raise ValueError(f'mark_trainable(positions={positions!r}): {type(self).__name__} has no embed_positions table '
                             '(only the learned-position models ESM-1b / ESM-1v do)')
        if positions and getattr(self, 'quantization', None) is not None:
            raise NotImplementedError(f'mark_trainable(positions={positions!r}): the learned-position models do not train on a quantised model')
        L = len(self.layers)
        if layers is None:
            chosen = set(range(L))
        else:
            chosen = set()
            for i in layers:
                if not -L <= int(i) < L:
                    raise IndexError(f'mark_trainable: layer {i} of a model with {L} layers')
                chosen.add(int(i) % L)
        for i, layer in enumerate(self.layers):
            att = layer.self_attn
            lins = [getattr(att, p) for p in ('q', 'k', 'v', 'out')]
            if layer.final_activation == 'gelu':
                lins += [layer.final[1], layer.final[3]]
            else:
                lins += [layer.final[1].activation, layer.final[1].fc, layer.final[2]]
            lns = [att.norm, layer.final[0]] + ([att.layernorm_q, att.layernorm_k] if att.pre_layernorm else [])
            for lin in lins:
                lin = lin.layer if isinstance(lin, LoRA) else lin
                want = bool(projections) and i in chosen
                if want and not lin.weight.dtype.is_floating_point:
                    raise NotImplementedError(f'mark_trainable: layer {i} is stored quantised ({lin.weight.dtype}); training needs '
                                              'unquantised bfloat16 base weights')
                for p in (lin.weight, lin.bias):
                    if p is not None and (want or p.requires_grad):
                        p.requires_grad_(want)
            for ln in lns:
                for p in ln.parameters(recurse=False):
                    p.requires_grad_(bool(norms) and i in chosen)
        for ln in (self.emb_layer_norm_after, getattr(self, 'emb_layer_norm_before', None)):
            if ln is not None:
                for p in ln.parameters(recurse=False):
                    p.requires_grad_(bool(norms) and layers is None)
        if embedding:
            self.__dict__['_train_embedding'] = True
            self.embed_tokens.weight.requires_grad_(True)
        elif self.__dict__.pop('_train_embedding', False):
            self.embed_tokens.weight.requires_grad_(False)
        was = self.__dict__.pop('_train_positions', False)
        if positions:
            self.__dict__['_train_positions'] = positions
        if positions is True:
            pe.weight.requires_grad_(True)
        elif was is True:                                           # (the flag the opt-in had set; one set by hand is not touched)
            pe.weight.requires_grad_(False)
        return self

    def extend_positions(self, max_positions: int):
        """Only the learned-position models (ESM-1b / ESM-1v) have a position table to extend."""
        raise ValueError(f'extend_positions: {type(self).__name__} has no embed_positions table')

    # -- loading -------------------------------------------------------------------
    @classmethod
    def create_model(cls, path, checkpointing=False):
        """Model skeleton (meta tensors) from the checkpoint's metadata strings
        (esm.py:319-340)."""
        md = _read_metadata(path)
        name = md['name'].split('_')[0]
        assert name == cls.__name__.lower(), \
            f'Invalid weight for the {cls.__name__} model. ' \
            f'You are trying to load a {name} model weights to a {cls.__name__} model.'
        with torch.device('meta'):
            return cls(num_layers=int(md['num_layers']), embed_dim=int(md['embed_dim']),
                       attention_heads=int(md['attention_heads']), checkpointing=checkpointing)

    @classmethod
    def from_pretrained(cls, path, quantization=None, checkpointing=False, device='cpu'):
        """Load a safetensors checkpoint in the reference layout.
        The file's tensors become the parameters directly (no copy besides the H2D)."""
        assert quantization in {None, '8bit', '4bit', '8bitexperimental'}, \
            f'load_in must be one of [None, "8bit", "4bit"] but got {quantization}'
        if quantization is not None:
            assert device != 'cpu', 'Quantized model cannot be loaded on cpu provide CUDA gpu device'
        from safetensors.torch import load_file
        model = cls.create_model(path, checkpointing=checkpointing)
        dev = torch.device('cuda', device) if isinstance(device, int) else torch.device(device)
        state = load_file(path, device=str(dev))
        contact = {k: state.pop(k) for k in [k for k in state if k.startswith('contact_head.')]}
        model.load_state_dict(state, strict=True, assign=True)
        if any(k.endswith('regression.weight') for k in contact):      # the checkpoint carries a contact regression
            model.set_contact_head(contact)
        for p in model.parameters():
            p.requires_grad_(False)
        if quantization is not None:                    # weight-only storage formats (esme/quantization.py)
            from esme.quantization import quantize_model_
            quantize_model_(model, cls.quant_type_4bit if quantization == '4bit' else 'int8')
        return model.eval()


class ESMC(ESM2):
    alphabet = Alphabet3
    vocab_size = 64
    zero_mask_rows = False         # plain lookup (esm.py:876)

    def __init__(self, num_layers: int = 30, embed_dim: int = 960, attention_heads: int = 15,
                 checkpointing: bool = False, dropout: float = 0., dtype=torch.bfloat16):
        super().__init__(num_layers=num_layers, embed_dim=embed_dim, attention_heads=attention_heads,
                         checkpointing=checkpointing, rotary_embedding=True, dropout=dropout, dtype=dtype)

    def _make_layer(self, rotary_embedding, dropout, dtype):
        return FlashTransformerLayer(self.embed_dim, 8 / 3, self.attention_heads, rotary_embedding=True,
                                     pre_layernorm=True, bias=False, final_activation='swiglu',
                                     residue_scaling=math.sqrt(self.num_layers / 36), dropout=dropout, dtype=dtype)

    def _make_final_norm(self, dtype):
        return LayerNorm(self.embed_dim, bias=False, dtype=dtype)

    # `layers=` is validated against the model depth like ESM2.  (The reference's ESM-C compares against the
    # ARGUMENT list, esm.py:873 `i < len(layers)`, which rejects every useful tap such as layers=[30]; that typo is
    # deliberately not reproduced -- any call the reference accepts is accepted here with the same result.)


class _LearnedPositionESM(ESM2):
    """Shared part of ESM-1b / ESM-1v (reference esme/esm.py:618-735): ESM-2's transformer stack without
    rotary, plus a learned position table added to the token embedding.  The reference fixes the size at
    33 x 1280 x 20; the dimensions are arguments here (same defaults) so small instances can be tested."""
    norm_before = False

    def __init__(self, checkpointing: bool = False, dtype=torch.bfloat16, num_layers: int = 33,
                 embed_dim: int = 1280, attention_heads: int = 20):
        super().__init__(num_layers=num_layers, embed_dim=embed_dim, attention_heads=attention_heads,
                         checkpointing=checkpointing, rotary_embedding=False, dtype=dtype)
        if self.norm_before:
            self.emb_layer_norm_before = LayerNorm(embed_dim, dtype=dtype)
        self.embed_positions = LearnedPositionalEmbedding(4096, embed_dim, dtype=dtype)

    def _embedding_phys(self, tokens, pad_args=None):
        """token rows (`<mask>` zeroed) + learned position rows [-> LayerNorm (ESM-1b)] -> `<pad>` rows zeroed
        (esm.py:634-652 / :694-711)."""
        assert not self.padded, 'learned-position models are built at 64-aligned widths'
        pe = self.embed_positions
        if tokens.ndim == 2:
            assert pad_args is None, 'pad_args must be None for esm1b with 2D tokens'
            idx, offset = pe.positions(tokens).to(torch.int32), 0
        elif tokens.ndim == 1:
            assert pad_args is not None, 'pad_args must be provided for esm1b with 1D tokens'
            cu_lens, max_len = pad_args
            if int(max_len) > pe.max_positions:
                raise ValueError(f'Sequence length {max_len} above maximum  sequence length of {pe.max_positions}')
            idx, offset = _hip.seq_positions(cu_lens, tokens.numel())[0], pe.padding_idx + 1
        else:
            raise ValueError('tokens must be 1D or 2D for esm1v')
        x = _hip.embed_positions(tokens, self.embed_tokens.weight, pe.weight, idx, offset,
                                 mask_idx=self.alphabet.mask_idx)
        if self.norm_before:
            x2 = x.view(-1, x.shape[-1])
            self.emb_layer_norm_before(x2, out=x2)
        if tokens.ndim == 2:
            x.masked_fill_(tokens.eq(self.alphabet.padding_idx).unsqueeze(-1), 0.0)   # row selection, no arithmetic
        return x

    def extend_positions(self, max_positions: int):
        """Replace `embed_positions` by a table for sequences of up to `max_positions` tokens: a new LearnedPositionalEmbedding of the
        same dtype and device whose first rows are the old table, bit for bit, and whose other rows are zeros -- how the run that made
        the 4 096-position checkpoints started from the released 1 024-position tables; train the new rows with
        mark_trainable(False, False, positions=True).  requires_grad is carried over; captured graphs, the C-entry descriptor and
        every derived weight copy are dropped, since they hold the old table.  ValueError when the table would shrink.  Returns self."""
        old = self.embed_positions
        max_positions = int(max_positions)
        if max_positions < old.max_positions:
            raise ValueError(f'extend_positions: cannot shrink the position table from {old.max_positions} to {max_positions} positions')
        if max_positions == old.max_positions:
            return self
        w = old.weight
        with torch.device(w.device):
            new = LearnedPositionalEmbedding(max_positions, old.embedding_dim, dtype=w.dtype)
        with torch.no_grad():
            new.weight[:old.num_embeddings].copy_(w)
        new.weight.requires_grad_(w.requires_grad)
        self.embed_positions = new.train(self.training)
        self.invalidate_graphs()
        return self

    def _embedding_exact(self, x, tokens, pad_args, pad_indices):
        """token row + learned-position row summed in fp32 [-> emb_layer_norm_before in fp32 (ESM-1b)] -> `<pad>` rows zeroed: what
        the reference's fp32 forward starts from (the bf16 path rounds the sum, and ESM-1b's LayerNorm output, to bf16)."""
        pe = self.embed_positions
        if tokens.ndim == 2:
            idx, offset = pe.positions(tokens).to(torch.int32), 0
        else:
            idx, offset = _hip.seq_positions(pad_args[0], tokens.numel())[0], pe.padding_idx + 1
        x32 = _hip.embed_positions(tokens, self.embed_tokens.weight, pe.weight, idx, offset, mask_idx=self.alphabet.mask_idx, f32=True)
        x32 = x32.view(-1, x32.shape[-1])
        if self.norm_before:
            ln = self.emb_layer_norm_before
            scratch = torch.empty(x32.shape[0], 2 * x32.shape[1], dtype=torch.bfloat16, device=x32.device)
            _hip.layernorm_split(x32, ln.weight, ln.bias, ln.eps, x32.shape[1], out=scratch, out32=x32)      # fp32 result in place
        if tokens.ndim == 2:               # (B, S) grid: zero the `<pad>` rows, then keep the rows unpad_input keeps (16-byte chunk copies)
            x32.masked_fill_(tokens.reshape(-1, 1).eq(self.alphabet.padding_idx), 0.0)
            x32 = _hip.gather_rows(x32.view(torch.bfloat16), pad_indices).view(torch.float32)
        return x32

    @classmethod
    def create_model(cls, path, checkpointing=False):
        md = _read_metadata(path)
        name = md['name'].split('_')[0]
        assert name == cls.__name__.lower(), \
            f'Invalid weight for the {cls.__name__} model. ' \
            f'You are trying to load a {name} model weights to a {cls.__name__} model.'
        from safetensors import safe_open
        with safe_open(path, framework='pt', device='cpu') as f:      # a table written after extend_positions() has more rows
            rows = f.get_slice('embed_positions.weight').get_shape()[0]
        with torch.device('meta'):
            model = cls(checkpointing=checkpointing, num_layers=int(md.get('num_layers', 33)),
                        embed_dim=int(md.get('embed_dim', 1280)), attention_heads=int(md.get('attention_heads', 20)))
            if rows != model.embed_positions.num_embeddings:
                model.embed_positions = LearnedPositionalEmbedding(rows - 2, model.embed_dim, dtype=model.embed_positions.weight.dtype)
        return model


class ESM1b(_LearnedPositionESM):
    norm_before = True


class ESM1v(_LearnedPositionESM):
    norm_before = False
