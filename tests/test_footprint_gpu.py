"""Every device-pointer entry point of include/esme_hip.h inside guard-banded arenas (tests/footprint.py): write containment, read
independence (NaN against zero guards), layout invariance (arena views against contiguous tensors) and uninitialised workspaces.

What a green run does and does not prove:
 - it proves that no write lands outside an operand within the bands (256 rows of the operand's ld, 64 columns);
 - it proves that no value outside an operand, or in a workspace's previous contents, can reach an output through arithmetic;
 - it does NOT see a stray read whose value is discarded by a select, nor an access beyond the bands.

Coverage (every exported function that takes a pointer; test_footprint_cpu.py fails when one is missing here or has no case):

  entry point                                  forms covered
  esme_hip_gemm_bf16                           none / no bias / GELU / residual (in place) / SwiGLU; M 1, 255, 257; N 8, 72, 264, 520; K 64, 2048; scalar-epilogue fallbacks (ldc % 8 != 0; ldr % 8 != 0 with an 8-byte aligned resid; N % 8 != 0)
  esme_hip_gemm_bf16_fused                     LN fold (+ GELU, + rotary, q_scale), stats_out, resid32, out32 (c32), split operand + pair output, fp16 forms: pair stream in
                                               place with pair_scale_in / _out, extension K-tile, col_absmax; LN fold + ext tile + rotary + qk_sumsq; q / k pair output; LoRA [x | u] column view
  esme_hip_gemm_bf16_opts                      the forms above under tile 1 / 2 x persist 0 / 1, incl. M = 170 * 256 + 1 (513 tiles: one more than two persistent walks) and the scalar-epilogue
                                               fallbacks (ldc / ldr % 8 != 0: held to the float64 bound; with persist 1 the launcher leaves the persistent kernel)
  esme_hip_gemm_qkv_rotary                     head dims 16 / 32 / 64
  esme_hip_gemm_stats_blocks_opts              host pointer only (opts struct): called by every stats_out case under options
  esme_hip_attn_varlen_fwd                     head dims 16 / 32 / 64 / 128, q / k / v column views of one (T, 3E) arena, lengths 1, 31, 33, 127, 129, 257, 1; o with ld_o % 8 == 4 and an
                                               8-byte aligned base (head dims 64 / 32 fall to the generic kernel: held to the float64 bound)
  esme_hip_attn_varlen_fwd_opts                every (variant, speculative, q_blocks) of the error-bound tests, bf16 and fp16, prescaled and fixed-reference forms, a
                                               batch whose work items are redone, with and without seq_order (order and cu_lens in arenas of their own)
  esme_hip_attn_varlen_fwd_exact               head dims 16 / 32 / 64 / 128
  esme_hip_attn_varlen_fwd_split               head dims 16 / 32 / 64 / 128, with and without seq_order
  esme_hip_attn_varlen_fwd_qkpair_f16          head dims 16 / 32 / 64, with and without seq_order
  esme_hip_attn_varlen_fwd_qkpair_f16_opts     variants 0 / 1 / 2
  esme_hip_layernorm                           T 1 / 37, E 64 / 1280 / 5120, with and without bias
  esme_hip_layernorm_f32                       the same
  esme_hip_layernorm_split                     fp32 / bf16-pair / fp16-pair input, y32
  esme_hip_layernorm_split_checked             the same with the overflow flag
  esme_hip_rotary_varlen, esme_hip_rotary_varlen_f16     head dims 16 / 32 / 64 / 128, q / k column views, first and last table row
  esme_hip_rotary_split, esme_hip_rotary_split_f16       pair q / k blocks, fp32 tables
  esme_hip_qk_norm_rotary, esme_hip_qk_norm_rotary_scaled, esme_hip_qk_norm_rotary_f16, esme_hip_qk_norm_rotary_f16_guarded,
  esme_hip_qk_norm_rotary_f16_scaled           head dims 64 / 32 with the guard maxima (qk_sumsq)
  esme_hip_residual_f32                        init 0 / 1, sums
  esme_hip_stream_operand, esme_hip_stream_operand_scaled, esme_hip_stream_operand_guarded     bf16 / fp16 single, pair, scaled pair with extension tile and col_absmax
  esme_hip_pair_to_f32                         bf16 and fp16 pairs
  esme_hip_row_sums                            T 1 / 37
  esme_hip_softmax_rows, esme_hip_softmax_rows_f32       V 33 / 64, softmax and log-softmax
  esme_hip_embed                               smallest and largest token id, mask and pad rows
  esme_hip_embed_positions, esme_hip_embed_positions_f32 smallest / largest token id and position (first and last table rows)
  esme_hip_seq_positions, esme_hip_seq_order   1-row sequences first and last
  esme_hip_gather_rows, esme_hip_scatter_rows  indices 0 and rows - 1, out-of-range indices
  esme_hip_segment_mean                        bf16 / fp32, empty sequences first, in the middle and last
  esme_hip_attn_pool_fold, esme_hip_attn_pool  bf16 / fp32, exact-size workspace, an empty sequence
  esme_hip_relu_linear                         bf16 / fp32
  esme_hip_lora_down, esme_hip_lora_down_ln    u as the columns E .. E + X - 1 of the buffer that holds x
  esme_hip_quantize_4bit, esme_hip_dequantize_4bit, esme_hip_quantize_8bit, esme_hip_dequantize_8bit     N * K on and off a 256-element boundary, col_scale
  esme_hip_forward, esme_hip_forward_workspace_bytes                 synthetic ESM-2, ESM-C and padded ESM2-35M-like models; x, logits and the exact-size workspace in arenas
  esme_hip_forward_half, esme_hip_forward_half_workspace_bytes       the same models; x32, pair, rep32 and the workspace in arenas
  esme_hip_forward_exact, esme_hip_forward_exact_workspace_bytes     the same; the workspace zeroed for the padded model (as the header demands), poisoned otherwise

No form is skipped.
"""
import contextlib
import ctypes
import dataclasses
import os
import tempfile
from typing import Callable, Tuple

import pytest
import torch

import footprint as fp
from footprint import Case, Operand

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF, H16, F32, I32, I64 = torch.bfloat16, torch.float16, torch.float32, torch.int32, torch.int64
LOG2E = 1.4426950408889634


@dataclasses.dataclass
class Spec:
    id: str
    symbols: Tuple[str, ...]
    build: Callable[[], Case]


CASES = []


def add(id, symbols, build):
    CASES.append(Spec(id, tuple('esme_hip_' + s for s in symbols.split()), build))


def rnd(shape, seed, scale=1.0, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def P(t):
    return t.data_ptr() if t is not None else None


def call_c(name, *args):
    from esme import _hip
    _hip._check(getattr(_hip.load(), name)(*args, _hip._stream()), name)


def out(name, shape, dtype=BF, **kw):
    return Operand(name, torch.empty(shape, dtype=dtype), 'out', **kw)


# ------------------------------------------------------------------ GEMM

def gemm_case(form, M, N, K, tile=0, persist=-1, entry='opts'):
    """entry: 'opts' (esme_hip_gemm_bf16_opts under gemm_options), 'fused' (esme_hip_gemm_bf16_fused), 'plain' (esme_hip_gemm_bf16 /
    esme_hip_gemm_qkv_rotary)."""
    from esme import _hip
    f16 = form.startswith('f16')
    dt = H16 if f16 else BF
    ops = [Operand('A', rnd((M, K), 1, dtype=dt)), Operand('W', rnd((N, K), 2, K ** -0.5).to(dt), pad=False), Operand('bias', rnd((N,), 3, 0.5))]
    n_out = N // 2 if form == 'swiglu' else N
    lengths = [1, M - 1] if M > 1 else [1]
    H = 0

    def rot_ops(d, tdt):
        nonlocal H
        H = N // 3 // d
        from oracle import esm_oracle as O
        cos, sin = O.rotary_tables(max(lengths), d, F32)
        pos = torch.cat([torch.arange(n, dtype=I32) for n in lengths])
        return [Operand('cos', cos.to(tdt).contiguous(), pad=False), Operand('sin', sin.to(tdt).contiguous(), pad=False), Operand('pos', pos)]

    def ln_ops(dim=None):
        a = ops[0].data[:, :dim or K].double()
        sums = torch.stack((a.sum(1), (a * a).sum(1)), 1).float()
        return [Operand('sums', sums, pad=False), Operand('c1', rnd((N,), 5, 1.0, F32)), Operand('c2', rnd((N,), 6, 1.0, F32))]

    ln_dim = K - 64 if form in ('f16_ln_ext_rotary', 'f16_qk_pair') else K            # the extension K-tile is not part of the LayerNorm
    if form in ('none', 'gelu', 'swiglu', 'f16_none', 'scalar_fallback'):
        ops.append(out('C', (M, n_out), dt, **({'ld': n_out + 129, 'lead': 64} if form == 'scalar_fallback' else {})))
    elif form == 'scalar_resid':                  # ldr % 8 != 0 and a resid base that is only 8-byte aligned: scalar residual loads + 2-byte stores (C itself 16-byte addressable)
        ops += [Operand('resid', rnd((M, N), 4), ld=N + 132, lead=68), out('C', (M, N))]
    elif form == 'nobias':
        ops.append(out('C', (M, N), dt))
    elif form == 'residual':
        ops += [Operand('resid', rnd((M, N), 4)), out('C', (M, N))]
    elif form == 'residual_inplace':
        ops.append(Operand('C', rnd((M, N), 4), 'inout'))
    elif form == 'stats':
        ops += [Operand('resid', rnd((M, N), 4)), out('C', (M, N))]
    elif form == 'resid32':
        ops += [Operand('x32', rnd((M, N), 4, 2.0, F32), 'inout'), out('C', (M, N))]
    elif form in ('ln_fold', 'ln_fold_gelu'):
        ops += ln_ops() + [out('C', (M, N))]
    elif form in ('rotary', 'rotary_qscale', 'ln_fold_rotary'):
        ops += rot_ops({576: 64, 384: 32, 192: 16}[N], BF) + (ln_ops() if form == 'ln_fold_rotary' else []) + [out('C', (M, N))]
    elif form == 'out32':
        ops[0] = Operand('A', rnd((M, 2 * K), 1))
        ops.append(out('C32', (M, N), F32))
    elif form in ('split_pair', 'split_pair_gelu'):
        ops[0] = Operand('A', rnd((M, 2 * K), 1))
        ops.append(out('C', (M, 2 * N)))
    elif form == 'f16_pair_stream':               # [hi | ext (64) | lo], scaled, 3 extension columns, the plan guard's column maxima
        x = rnd((M, N), 7, 3.0, F32)
        hi = x.to(H16)
        pair = torch.zeros(M, 2 * N + 64, dtype=H16)
        pair[:, :N], pair[:, N + 64:] = hi, (x - hi.float()).to(H16)
        ops += [Operand('pair', pair, 'inout'), Operand('si', 0.75 + 0.5 * torch.rand(N, generator=torch.Generator().manual_seed(8))),
                Operand('so', 0.75 + 0.5 * torch.rand(N, generator=torch.Generator().manual_seed(9))),
                Operand('sel', torch.tensor([3, N // 2, N - 1], dtype=I32)), Operand('absmax', torch.zeros(N, dtype=I32), 'inout')]
    elif form in ('f16_ln_ext_rotary', 'f16_qk_pair'):     # A = [hi | ext] (K = E + 64) as a column view of the pair stream [hi | ext | lo]
        E = K - 64
        ops[0] = Operand('stream', rnd((M, 2 * E + 64), 1, dtype=H16))
        ops += rot_ops(64, F32 if form == 'f16_qk_pair' else H16) + ln_ops(E)
        if form == 'f16_qk_pair':
            ops.append(out('C', (M, N + 512), H16))
        else:
            ops += [out('C', (M, N), H16), Operand('sumsq', torch.zeros(2 * H, dtype=I32), 'inout')]
    elif form == 'lora_xu':                       # the operand row [x | u] with lda wider than K + X: A is a column view
        ops[0] = Operand('xu', rnd((M, K + 128), 1))
        ops[1] = Operand('W', torch.cat((ops[1].data, rnd((N, 64), 9, K ** -0.5)), 1).contiguous(), pad=False)      # [W | s B] (N, K + X), X = 64
        ops.append(out('C', (M, N)))
    else:
        raise KeyError(form)

    def call(v):
        a, w, b = v.get('A'), v['W'], v['bias']
        with (_hip.gemm_options(tile=tile, persist=persist) if entry == 'opts' else contextlib.nullcontext()):
            ln = (v['sums'].view(1, M, 2), ln_dim, 1e-5, v['c1'], v['c2']) if 'sums' in v else None
            rot = (v['cos'], v['sin'], v['pos'], v['cos'].shape[1], 2 * (N // 3)) if 'cos' in v else None
            if form in ('none', 'gelu', 'swiglu', 'nobias', 'scalar_fallback') and entry == 'plain':
                _hip.gemm(a, w, None if form == 'nobias' else b, {'gelu': _hip.EPI_GELU, 'swiglu': _hip.EPI_SWIGLU}.get(form, 0), out=v['C'])
            elif form in ('none', 'gelu', 'swiglu', 'nobias', 'f16_none', 'scalar_fallback'):
                _hip.gemm_fused(a, w, None if form == 'nobias' else b, {'gelu': _hip.EPI_GELU, 'swiglu': _hip.EPI_SWIGLU}.get(form, 0), out=v['C'])
            elif form in ('residual', 'scalar_resid'):
                (_hip.gemm if entry == 'plain' else _hip.gemm_fused)(a, w, b, _hip.EPI_RESIDUAL, resid=v['resid'], alpha=0.75, out=v['C'])
            elif form == 'residual_inplace':
                (_hip.gemm if entry == 'plain' else _hip.gemm_fused)(a, w, b, _hip.EPI_RESIDUAL, resid=v['C'], alpha=0.75, out=v['C'])
            elif form == 'stats':
                _hip.gemm_fused(a, w, b, _hip.EPI_RESIDUAL, resid=v['resid'], alpha=0.5, out=v['C'], stats_out=v['stats'])
            elif form == 'resid32':
                _hip.gemm_fused(a, w, b, _hip.EPI_RESIDUAL, None, 0.5, out=v['C'], resid32=v['x32'])
            elif form in ('ln_fold', 'ln_fold_gelu'):
                _hip.gemm_fused(a, w, None, _hip.EPI_GELU if form == 'ln_fold_gelu' else 0, out=v['C'], ln=ln)
            elif form == 'rotary' and entry == 'plain':
                _hip.gemm_qkv_rotary(a, w, b, v['cos'], v['sin'], v['pos'], rot[3], rot[4], out=v['C'])
            elif form in ('rotary', 'rotary_qscale', 'ln_fold_rotary'):
                _hip.gemm_fused(a, w, None if ln else b, out=v['C'], ln=ln, rot=rot, q_scale=0.125 * LOG2E if form == 'rotary_qscale' else 0.0)
            elif form == 'out32':
                _hip.gemm_fused(a, w, b, split_a=True, out32=v['C32'])
            elif form in ('split_pair', 'split_pair_gelu'):
                _hip.gemm_fused(a, w, b, _hip.EPI_GELU if form.endswith('gelu') else 0, out=v['C'], split_a=True, pair_out=True)
            elif form == 'f16_pair_stream':
                _hip.gemm_fused(a, w, b, _hip.EPI_RESIDUAL, None, 0.7, resid_pair=v['pair'], pair_scale=(v['si'], v['so']), pair_ext=v['sel'], col_absmax=v['absmax'])
            elif form == 'f16_ln_ext_rotary':
                _hip.gemm_fused(v['stream'][:, :K], w, None, out=v['C'], ln=ln, rot=rot, q_scale=0.125 * LOG2E, qk_sumsq=v['sumsq'])
            elif form == 'f16_qk_pair':
                _hip.gemm_fused(v['stream'][:, :K], w, None, out=v['C'], ln=ln, rot=rot, pair_out=True, pair_cols=512)
            elif form == 'lora_xu':
                _hip.gemm_fused(v['xu'][:, :K + 64], w, b, out=v['C'])

    if form == 'stats':
        with (_hip.gemm_options(tile=tile, persist=persist) if entry == 'opts' else contextlib.nullcontext()):
            nblk = _hip.stats_blocks(M, N)
        ops.append(out('stats', (nblk * M, 2), F32, pad=False))
    case = Case(f'gemm {form} {M}x{N}x{K} tile{tile} persist{persist} {entry}', ops, call)
    if form in ('scalar_fallback', 'scalar_resid'):
        # ldc % 8 != 0 (scalar_resid: ldr % 8 != 0 and an 8-byte aligned resid) sends the ARENA run through the 2-byte epilogue -- and, under persist = 1,
        # off the persistent kernel -- while the contiguous run keeps the 16-byte one: same accumulators, same rounding -- held to the project's bound
        # for this GEMM (error_bounds.gemm_reference) instead of bit equality.  (N % 8 != 0 takes the 2-byte epilogue in BOTH layouts: those cases,
        # form 'none' with N = 68, stay bit-equal.)
        def cmp(name, got, ref):
            import error_bounds as eb
            a_, w_, b_ = (o.data.to(DEV) for o in ops[:3])
            if form == 'scalar_resid':
                r, bound, _ = eb.gemm_reference(a_, w_, b_, 'residual', resid=ops[3].data.to(DEV), alpha=0.75)
            else:
                r, bound, _ = eb.gemm_reference(a_, w_, b_)
            eb.assert_bounded(got.view(BF).to(DEV), r, bound, 'scalar-epilogue fallback in an arena')
            eb.assert_bounded(ref.view(BF).to(DEV), r, bound, 'vector epilogue on contiguous tensors')
        case.plain_compare = cmp
    return case


CFG = [(1, 0), (1, 1), (2, 0), (2, 1)]
for _t, _p in CFG:
    for _form, _M, _N, _K in [('none', 257, 520, 64), ('nobias', 255, 72, 2048), ('gelu', 1, 264, 64), ('residual', 257, 264, 2048), ('residual_inplace', 255, 520, 64),
                              ('swiglu', 257, 576, 64), ('none', 255, 8, 2048), ('ln_fold', 257, 264, 320), ('ln_fold_gelu', 255, 520, 64), ('rotary', 257, 576, 64),
                              ('rotary_qscale', 255, 384, 320), ('rotary', 257, 192, 64), ('ln_fold_rotary', 257, 576, 320), ('stats', 257, 576, 64), ('resid32', 255, 264, 2048),
                              ('out32', 257, 72, 64), ('split_pair', 257, 264, 64), ('split_pair_gelu', 255, 520, 128), ('f16_none', 257, 520, 64),
                              ('f16_pair_stream', 257, 320, 128), ('f16_ln_ext_rotary', 257, 768, 320), ('f16_qk_pair', 255, 768, 320), ('lora_xu', 257, 264, 320),
                              ('scalar_fallback', 257, 72, 64), ('scalar_resid', 255, 72, 2048), ('none', 257, 68, 64), ('residual', 255, 68, 64)]:
        add(f'gemm-{_form}-{_M}x{_N}x{_K}-tile{_t}-persist{_p}', 'gemm_bf16_opts' + (' gemm_stats_blocks_opts' if _form == 'stats' else ''),
            lambda f=_form, M=_M, N=_N, K=_K, t=_t, p=_p: gemm_case(f, M, N, K, t, p))
# one more tile than two walks of the 256 persistent workgroups: 171 x 3 = 513 tiles of 256 x 256, the last row tile one row deep
# (scalar_fallback: with ldc % 8 != 0 the launcher leaves the persistent kernel for one workgroup per tile)
for _form in ('none', 'residual_inplace', 'stats', 'resid32', 'scalar_fallback'):
    add(f'gemm-{_form}-43521x{576 if _form == "stats" else 520}x64-tile2-persist1', 'gemm_bf16_opts',
        lambda f=_form: gemm_case(f, 170 * 256 + 1, 576 if f == 'stats' else 520, 64, 2, 1))
for _form, _M, _N, _K in [('none', 257, 520, 64), ('gelu', 255, 72, 2048), ('nobias', 1, 8, 64), ('residual', 257, 264, 64), ('residual_inplace', 255, 520, 2048),
                          ('swiglu', 257, 576, 64), ('scalar_fallback', 257, 72, 64), ('scalar_resid', 257, 72, 64), ('none', 255, 68, 2048)]:
    add(f'gemm_bf16-{_form}-{_M}x{_N}x{_K}', 'gemm_bf16', lambda f=_form, M=_M, N=_N, K=_K: gemm_case(f, M, N, K, entry='plain'))
for _N in (576, 384, 192):
    add(f'gemm_qkv_rotary-257x{_N}x64', 'gemm_qkv_rotary', lambda N=_N: gemm_case('rotary', 257, N, 64, entry='plain'))
for _form, _M, _N, _K in [('ln_fold', 257, 264, 320), ('stats', 255, 576, 64), ('resid32', 257, 520, 64), ('out32', 255, 72, 2048), ('split_pair', 257, 264, 64),
                          ('f16_pair_stream', 255, 320, 128), ('f16_ln_ext_rotary', 257, 768, 320), ('f16_qk_pair', 257, 768, 320), ('lora_xu', 255, 72, 320),
                          ('rotary_qscale', 257, 576, 64)]:
    add(f'gemm_fused-{_form}-{_M}x{_N}x{_K}', 'gemm_bf16_fused', lambda f=_form, M=_M, N=_N, K=_K: gemm_case(f, M, N, K, entry='fused'))


# ------------------------------------------------------------------ attention

LENGTHS = [1, 31, 33, 127, 129, 257, 1]          # the first sequence starts at operand row 0, the last ends at its last row; 1-row sequences first and last


def cu_of(lengths):
    return torch.tensor([0] + list(torch.tensor(lengths).cumsum(0)), dtype=I32)


def order_of(lengths):
    return torch.tensor(sorted(range(len(lengths)), key=lambda i: -lengths[i]), dtype=I32)


def attn_case(d, H, dtype=BF, variant=None, spec=1, qb=0, entry='opts', prescaled=False, exact=False, lengths=LENGTHS, scale=1.5, seed=0, o_fallback=False):
    from esme import _hip
    T, E = sum(lengths), H * d
    qkv = rnd((T, 3 * E), 20 + d + seed, scale, F32)
    if prescaled:
        qkv[:, :E] *= d ** -0.5 * LOG2E
    # o_fallback: ld_o % 8 == 4 and an o base that is only 8-byte aligned -- accepted by the launcher, but head dims 64 / 32 then leave the
    # software-pipelined kernels for the generic one
    okw = {'ld': E + 132, 'lead': 68} if o_fallback else {}
    ops = [Operand('qkv', qkv.to(dtype)), Operand('cu_lens', cu_of(lengths)), Operand('order', order_of(lengths)), out('o', (T, E), dtype, **okw)]
    if entry == 'opts':
        ops.append(out('o_ordered', (T, E), dtype, **okw))

    def call(v):
        q, k, vv = v['qkv'][:, :E], v['qkv'][:, E:2 * E], v['qkv'][:, 2 * E:]
        if entry == 'fwd':
            _hip.attn_varlen(q, k, vv, v['cu_lens'], max(lengths), H, out=v['o'])
        elif entry == 'exact':
            _hip.attn_varlen(q, k, vv, v['cu_lens'], max(lengths), H, out=v['o'], exact=True)
        else:
            with _hip.attn_options(variant=variant or 0, spec=spec, q_blocks=qb):
                assert _hip._TLS.attn_opts is not None
                _hip.attn_varlen(q, k, vv, v['cu_lens'], max(lengths), H, out=v['o'], q_prescaled=prescaled, exact=exact and dtype == H16)
                _hip.attn_varlen(q, k, vv, v['cu_lens'], max(lengths), H, out=v['o_ordered'], q_prescaled=prescaled, exact=exact and dtype == H16, order=v['order'])
    case = Case(f'attention {entry} d{d} {dtype} variant {variant} spec {spec} qb {qb} prescaled {prescaled} o_fallback {o_fallback}', ops, call)
    if o_fallback:
        # another kernel in the arena (generic) than on contiguous tensors (software-pipelined): both held to the project's attention bound
        def cmp(name, got, ref):
            import error_bounds as eb
            x = ops[0].data.to(DEV)
            fmt = 'fp16' if dtype == H16 else 'bf16'
            r, bound, _ = eb.attention_reference(x[:, :E], x[:, E:2 * E], x[:, 2 * E:], cu_of(lengths).to(DEV), H, d ** -0.5, fmt, fmt)
            eb.assert_bounded(got.view(dtype).to(DEV), r, bound, f'{name}: generic kernel (ld_o % 8 != 0) in an arena')
            eb.assert_bounded(ref.view(dtype).to(DEV), r, bound, f'{name}: software-pipelined kernel on contiguous tensors')
        case.plain_compare = cmp
    return case


ATTN_BF16 = [(16, 8, 0, 1, 0), (32, 8, 0, 1, 0), (64, 4, 0, 1, 0), (128, 2, 0, 1, 0), (64, 4, 1, 0, 1), (64, 4, 1, 0, 2), (32, 8, 1, 0, 0), (128, 2, 1, 0, 0),
             (16, 8, 1, 0, 0), (64, 4, 4, 1, 0), (64, 4, 4, 0, 0), (64, 4, 8, 1, 0), (64, 4, 8, 0, 0), (64, 4, 2, 1, 0), (32, 8, 2, 1, 0)]
for _d, _H, _v, _s, _q in ATTN_BF16:
    add(f'attn_opts-bf16-d{_d}-v{_v}-s{_s}-q{_q}', 'attn_varlen_fwd_opts', lambda d=_d, H=_H, v=_v, s=_s, q=_q: attn_case(d, H, BF, v, s, q))
for _d, _H, _v in [(64, 4, 0), (64, 4, 4), (64, 4, 8), (32, 8, 0), (64, 4, 2)]:
    add(f'attn_opts-bf16-prescaled-d{_d}-v{_v}', 'attn_varlen_fwd_opts', lambda d=_d, H=_H, v=_v: attn_case(d, H, BF, v, prescaled=True))
for _d, _H in [(16, 8), (32, 8), (64, 4), (128, 2)]:
    add(f'attn_fwd-d{_d}', 'attn_varlen_fwd', lambda d=_d, H=_H: attn_case(d, H, entry='fwd'))
    add(f'attn_exact-d{_d}', 'attn_varlen_fwd_exact', lambda d=_d, H=_H: attn_case(d, H, entry='exact'))
    add(f'attn_opts-f16-d{_d}', 'attn_varlen_fwd_opts', lambda d=_d, H=_H: attn_case(d, H, H16, scale=1.0))
    add(f'attn_opts-f16-exact-d{_d}', 'attn_varlen_fwd_opts', lambda d=_d, H=_H: attn_case(d, H, H16, exact=True, scale=1.0))
    if _d in (32, 64):
        add(f'attn_opts-f16-fixed-reference-d{_d}', 'attn_varlen_fwd_opts', lambda d=_d, H=_H: attn_case(d, H, H16, prescaled=True, scale=1.0))
for _d, _H in [(64, 4), (32, 8)]:
    add(f'attn_fwd-o-pitch-fallback-d{_d}', 'attn_varlen_fwd', lambda d=_d, H=_H: attn_case(d, H, entry='fwd', o_fallback=True))
    add(f'attn_opts-o-pitch-fallback-d{_d}-v2', 'attn_varlen_fwd_opts', lambda d=_d, H=_H: attn_case(d, H, BF, 2, o_fallback=True))
    add(f'attn_opts-f16-o-pitch-fallback-d{_d}', 'attn_varlen_fwd_opts', lambda d=_d, H=_H: attn_case(d, H, H16, scale=1.0, o_fallback=True))
# scores far above the fixed reference's window: the work items are redone with exact maxima
add('attn_opts-f16-fixed-reference-redo', 'attn_varlen_fwd_opts', lambda: attn_case(64, 4, H16, prescaled=True, scale=4.0, seed=5))


def attn_pair_case(kind, d, H, variant=None):
    from esme import _hip
    T, E = sum(LENGTHS), H * d
    if kind == 'split':
        x = rnd((T, 3 * E), 30 + d, 1.5, F32)
        hi = x.to(BF)
        data, ow, dt = torch.cat((hi, (x - hi.float()).to(BF)), 1).contiguous(), 2 * E, BF
    else:
        qk = rnd((T, 2 * E), 31 + d, 3.0, F32)
        hi = qk.to(H16)
        data, ow, dt = torch.cat((hi, rnd((T, E), 32, dtype=H16), (qk - hi.float()).to(H16)), 1).contiguous(), E, H16
    ops = [Operand('qkv', data), Operand('cu_lens', cu_of(LENGTHS)), Operand('order', order_of(LENGTHS)), out('o', (T, ow), dt), out('o_ordered', (T, ow), dt)]

    def call(v):
        q = v['qkv']
        cu, ml = v['cu_lens'], max(LENGTHS)
        if kind == 'split':
            _hip.attn_varlen_split(q, cu, ml, H, d, d ** -0.5, out=v['o'])
            _hip.attn_varlen_split(q, cu, ml, H, d, d ** -0.5, out=v['o_ordered'], order=v['order'])
        elif kind == 'qkpair':
            for o, order in ((v['o'], None), (v['o_ordered'], v['order'])):
                call_c('esme_hip_attn_varlen_fwd_qkpair_f16', P(q), P(q) + 2 * E, P(q) + 4 * E, q.stride(0), 3 * E, P(o), o.stride(0), P(cu), len(LENGTHS), T, H, d, ml,
                       d ** -0.5, P(order))
        else:
            with _hip.attn_options(variant=variant):
                _hip.attn_varlen_qkpair(q, cu, ml, H, d, d ** -0.5, out=v['o'])
                _hip.attn_varlen_qkpair(q, cu, ml, H, d, d ** -0.5, out=v['o_ordered'], order=v['order'])
    return Case(f'attention {kind} d{d} variant {variant}', ops, call)


for _d, _H in [(16, 8), (32, 8), (64, 4), (128, 2)]:
    add(f'attn_split-d{_d}', 'attn_varlen_fwd_split', lambda d=_d, H=_H: attn_pair_case('split', d, H))
    if _d != 128:
        add(f'attn_qkpair-d{_d}', 'attn_varlen_fwd_qkpair_f16', lambda d=_d, H=_H: attn_pair_case('qkpair', d, H))
for _d, _H, _v in [(16, 8, 0), (16, 8, 1), (32, 8, 0), (32, 8, 1), (32, 8, 2), (64, 4, 0), (64, 4, 1), (64, 4, 2)]:
    add(f'attn_qkpair_opts-d{_d}-v{_v}', 'attn_varlen_fwd_qkpair_f16_opts', lambda d=_d, H=_H, v=_v: attn_pair_case('qkpair_opts', d, H, v))


# ------------------------------------------------------------------ row operations

def ln_case(kind, T, E, bias=True):
    """kind: bf16, f32, split (fp32 in), split_pair (bf16 pair in), split_checked (fp16 pair in + flag)."""
    w, b = (1 + 0.1 * torch.randn(E, generator=torch.Generator().manual_seed(1))).to(BF), rnd((E,), 2, 0.05)
    ops = [Operand('w', w), Operand('b', b)]
    if kind == 'bf16':
        ops += [Operand('x', rnd((T, E), 3, 1.5)), out('y', (T, E))]
    elif kind == 'f32':
        ops += [Operand('x', rnd((T, E), 3, 1.5, F32)), out('y', (T, E))]
    elif kind == 'split':
        ops += [Operand('x', rnd((T, E), 3, 1.5, F32)), out('y', (T, 2 * E)), out('y32', (T, E), F32)]
    else:
        ops += [Operand('x', rnd((T, 2 * E), 3, 1.5, BF if kind == 'split_pair' else H16)), out('y', (T, 2 * E)), out('y32', (T, E), F32),
                Operand('flag', torch.zeros(1, dtype=I32), 'inout')]

    def call(v):
        x, y, bp = v['x'], v['y'], P(v['b']) if bias else None
        if kind in ('bf16', 'f32'):
            call_c('esme_hip_layernorm' if kind == 'bf16' else 'esme_hip_layernorm_f32', P(x), x.stride(0), P(v['w']), bp, P(y), y.stride(0), T, E, 1e-5)
        elif kind == 'split':
            call_c('esme_hip_layernorm_split', P(x), x.stride(0), 0, 0, P(v['w']), bp, P(y), y.stride(0), E, P(v['y32']), v['y32'].stride(0), T, E, 1e-5)
        elif kind == 'split_pair':
            call_c('esme_hip_layernorm_split', P(x), x.stride(0), 1, E, P(v['w']), bp, P(y), y.stride(0), E, P(v['y32']), v['y32'].stride(0), T, E, 1e-5)
        else:
            call_c('esme_hip_layernorm_split_checked', P(x), x.stride(0), 2, E, P(v['w']), bp, P(y), y.stride(0), E, P(v['y32']), v['y32'].stride(0), T, E, 1e-5, P(v['flag']))
    return Case(f'layernorm {kind} T{T} E{E} bias {bias}', ops, call)


for _T, _E, _b in [(1, 64, True), (37, 1280, False), (37, 5120, True), (1, 5120, True), (37, 64, True)]:
    add(f'layernorm-bf16-T{_T}-E{_E}', 'layernorm', lambda T=_T, E=_E, b=_b: ln_case('bf16', T, E, b))
    add(f'layernorm-f32-T{_T}-E{_E}', 'layernorm_f32', lambda T=_T, E=_E, b=_b: ln_case('f32', T, E, b))
    add(f'layernorm-split-T{_T}-E{_E}', 'layernorm_split', lambda T=_T, E=_E, b=_b: ln_case('split', T, E, b))
    add(f'layernorm-split-pair-T{_T}-E{_E}', 'layernorm_split', lambda T=_T, E=_E, b=_b: ln_case('split_pair', T, E, b))
    add(f'layernorm-split-checked-T{_T}-E{_E}', 'layernorm_split_checked', lambda T=_T, E=_E, b=_b: ln_case('split_checked', T, E, b))

ROT_LENGTHS = [1, 31, 129, 1]


def rot_pos():
    return torch.cat([torch.arange(n, dtype=I32) for n in ROT_LENGTHS])          # position 0 and max_len - 1: the first and last table rows


def rotary_case(kind, d, H):
    from oracle import esm_oracle as O
    T, E, ml = sum(ROT_LENGTHS), H * d, max(ROT_LENGTHS)
    cos, sin = O.rotary_tables(ml, d, F32)
    if kind in ('bf16', 'f16'):
        dt = BF if kind == 'bf16' else H16
        ops = [Operand('qkv', rnd((T, 3 * E), 4, dtype=dt), 'inout'), Operand('cos', cos.to(dt).contiguous(), pad=False), Operand('sin', sin.to(dt).contiguous(), pad=False),
               Operand('pos', rot_pos())]

        def call(v):
            q = v['qkv']
            call_c('esme_hip_rotary_varlen' + ('_f16' if kind == 'f16' else ''), P(q), P(q) + 2 * E, q.stride(0), P(v['cos']), P(v['sin']), P(v['pos']), T, H, d, ml)
    else:
        dt = BF if kind == 'split' else H16
        ops = [Operand('qkv', rnd((T, 6 * E), 4, dtype=dt), 'inout'), Operand('cos', cos.contiguous(), pad=False), Operand('sin', sin.contiguous(), pad=False),
               Operand('pos', rot_pos())]

        def call(v):
            q = v['qkv']
            call_c('esme_hip_rotary_split' + ('_f16' if kind == 'split_f16' else ''), P(q), q.stride(0), 3 * E, P(v['cos']), P(v['sin']), P(v['pos']), T, 2 * H, d, ml)
    return Case(f'rotary {kind} d{d}', ops, call)


for _d, _H in [(16, 8), (32, 8), (64, 4), (128, 2)]:
    add(f'rotary-bf16-d{_d}', 'rotary_varlen', lambda d=_d, H=_H: rotary_case('bf16', d, H))
    add(f'rotary-f16-d{_d}', 'rotary_varlen_f16', lambda d=_d, H=_H: rotary_case('f16', d, H))
    add(f'rotary-split-d{_d}', 'rotary_split', lambda d=_d, H=_H: rotary_case('split', d, H))
    add(f'rotary-split-f16-d{_d}', 'rotary_split_f16', lambda d=_d, H=_H: rotary_case('split_f16', d, H))


def qk_norm_case(form, d, H):
    from oracle import esm_oracle as O
    T, E, ml = sum(ROT_LENGTHS), H * d, max(ROT_LENGTHS)
    f16 = form.startswith('f16')
    dt = H16 if f16 else BF
    cos, sin = O.rotary_tables(ml, d, F32)
    g = torch.Generator().manual_seed(6)
    ops = [Operand('qkv', rnd((T, 3 * E), 5, dtype=dt), 'inout'), Operand('wq', (1 + 0.1 * torch.randn(E, generator=g)).to(BF)), Operand('wk', (1 + 0.1 * torch.randn(E, generator=g)).to(BF)),
           Operand('bq', rnd((E,), 7, 0.05)), Operand('bk', rnd((E,), 8, 0.05)), Operand('cos', cos.to(dt).contiguous(), pad=False), Operand('sin', sin.to(dt).contiguous(), pad=False),
           Operand('pos', rot_pos()), Operand('sumsq', torch.zeros(2 * H, dtype=I32), 'inout')]

    def call(v):
        q = v['qkv']
        args = [P(q), P(q) + 2 * E, q.stride(0), P(v['wq']), P(v['wk']), P(v['bq']), P(v['bk']), 1e-5, P(v['cos']), P(v['sin']), P(v['pos']), T, H, d, ml]
        name, tail = {'bf16': ('esme_hip_qk_norm_rotary', []), 'bf16_scaled': ('esme_hip_qk_norm_rotary_scaled', [0.125 * LOG2E]), 'f16': ('esme_hip_qk_norm_rotary_f16', []),
                      'f16_guarded': ('esme_hip_qk_norm_rotary_f16_guarded', [P(v['sumsq'])]), 'f16_scaled': ('esme_hip_qk_norm_rotary_f16_scaled', [0.125 * LOG2E, P(v['sumsq'])])}[form]
        call_c(name, *args, *tail)
    return Case(f'qk_norm_rotary {form} d{d}', ops, call)


for _form, _sym in [('bf16', 'qk_norm_rotary'), ('bf16_scaled', 'qk_norm_rotary_scaled'), ('f16', 'qk_norm_rotary_f16'), ('f16_guarded', 'qk_norm_rotary_f16_guarded'),
                    ('f16_scaled', 'qk_norm_rotary_f16_scaled')]:
    for _d, _H in [(64, 15), (32, 8)]:
        add(f'qk_norm_rotary-{_form}-d{_d}', _sym, lambda f=_form, d=_d, H=_H: qk_norm_case(f, d, H))


def stream_case(kind, T, E):
    if kind.startswith('residual'):
        init = kind.endswith('init')
        ops = [Operand('x32', rnd((T, E), 1, 2.0, F32), 'out' if init else 'inout'), Operand('o', rnd((T, E), 2)), out('x16', (T, E)), out('sums', (T, 2), F32, pad=False)]

        def call(v):
            call_c('esme_hip_residual_f32', P(v['x32']), v['x32'].stride(0), P(v['o']), v['o'].stride(0), 0.5, int(init), P(v['x16']), v['x16'].stride(0), P(v['sums']), T, E)
    elif kind in ('operand_bf16', 'operand_f16', 'operand_pair'):
        dt = BF if kind == 'operand_bf16' else H16
        pair = kind == 'operand_pair'
        ops = [Operand('x32', rnd((T, E), 1, 2.0, F32)), out('x16', (T, 2 * E if pair else E), dt), out('sums', (T, 2), F32, pad=False)]

        def call(v):
            call_c('esme_hip_stream_operand', P(v['x32']), v['x32'].stride(0), P(v['x16']), v['x16'].stride(0), E if pair else 0, int(dt == H16), P(v['sums']), T, E)
    elif kind in ('operand_scaled', 'operand_guarded'):          # [hi | ext (64) | lo], scaled, extension tile of 3 columns (then zeros)
        ops = [Operand('x32', rnd((T, E), 1, 2.0, F32)), out('x16', (T, 2 * E + 64), H16), out('sums', (T, 2), F32, pad=False),
               Operand('scale', 0.75 + 0.5 * torch.rand(E, generator=torch.Generator().manual_seed(3))), Operand('sel', torch.tensor([0, E // 2, E - 1], dtype=I32)),
               Operand('absmax', torch.zeros(E, dtype=I32), 'inout')]

        def call(v):
            args = [P(v['x32']), v['x32'].stride(0), P(v['x16']), v['x16'].stride(0), E + 64, 1, P(v['scale']), P(v['sel']), 3, E, P(v['sums'])]
            if kind == 'operand_guarded':
                call_c('esme_hip_stream_operand_guarded', *args, P(v['absmax']), T, E)
            else:
                call_c('esme_hip_stream_operand_scaled', *args, T, E)
    elif kind in ('pair_to_f32_bf16', 'pair_to_f32_f16'):
        ops = [Operand('x', rnd((T, 2 * E + 64), 1, dtype=BF if kind.endswith('bf16') else H16)), out('out', (T, E), F32)]

        def call(v):
            call_c('esme_hip_pair_to_f32', P(v['x']), v['x'].stride(0), E + 64, int(kind.endswith('f16')), P(v['out']), v['out'].stride(0), T, E)
    elif kind == 'row_sums':
        ops = [Operand('x', rnd((T, E), 1)), out('sums', (T, 2), F32, pad=False)]

        def call(v):
            call_c('esme_hip_row_sums', P(v['x']), v['x'].stride(0), T, E, P(v['sums']))
    return Case(f'{kind} T{T} E{E}', ops, call)


for _T, _E in [(1, 64), (37, 1280), (259, 320)]:
    for _kind, _sym in [('residual', 'residual_f32'), ('residual_init', 'residual_f32'), ('operand_bf16', 'stream_operand'), ('operand_f16', 'stream_operand'),
                        ('operand_pair', 'stream_operand'), ('operand_scaled', 'stream_operand_scaled'), ('operand_guarded', 'stream_operand_guarded'),
                        ('pair_to_f32_bf16', 'pair_to_f32'), ('pair_to_f32_f16', 'pair_to_f32'), ('row_sums', 'row_sums')]:
        add(f'{_kind}-T{_T}-E{_E}', _sym, lambda k=_kind, T=_T, E=_E: stream_case(k, T, E))


def softmax_case(dt, V, log, T=37):
    ops = [Operand('x', rnd((T, V), 1, 3.0, dt)), out('y', (T, V), dt)]

    def call(v):
        call_c('esme_hip_softmax_rows_f32' if dt == F32 else 'esme_hip_softmax_rows', P(v['x']), v['x'].stride(0), P(v['y']), v['y'].stride(0), T, V, log)
    return Case(f'softmax_rows {dt} V{V} log{log}', ops, call)


for _V in (33, 64):
    for _log in (0, 1):
        add(f'softmax_rows-bf16-V{_V}-log{_log}', 'softmax_rows', lambda V=_V, l=_log: softmax_case(BF, V, l))
        add(f'softmax_rows-f32-V{_V}-log{_log}', 'softmax_rows_f32', lambda V=_V, l=_log: softmax_case(F32, V, l))


def embed_case(kind):
    V, E, Pn, T = 33, 320, 70, 41
    tok = torch.randint(0, V, (T,), generator=torch.Generator().manual_seed(1))
    tok[0], tok[-1], tok[5], tok[6] = 0, V - 1, 31, 1                       # the first and last table rows; a mask row and a pad row
    pos = torch.arange(T, dtype=I32)
    pos[0], pos[-1] = 0, Pn - 1 - 2                                          # (+ pos_offset 2): the first addressed and the last position row
    ops = [Operand('tokens', tok), Operand('table', rnd((V, E), 2), pad=False)]
    if kind == 'embed':
        ops.append(out('out', (T, E), pad=False))

        def call(v):
            call_c('esme_hip_embed', P(v['tokens']), P(v['table']), P(v['out']), T, E, V, 31, 1)
    else:
        ops += [Operand('pos_table', rnd((Pn, E), 3), pad=False), Operand('pos', pos), out('out', (T, E), F32 if kind == 'f32' else BF, pad=False)]

        def call(v):
            call_c('esme_hip_embed_positions_f32' if kind == 'f32' else 'esme_hip_embed_positions', P(v['tokens']), P(v['table']), P(v['pos_table']), P(v['pos']), 2, P(v['out']),
                   T, E, V, Pn, 31)
    return Case(f'embed {kind}', ops, call)


add('embed', 'embed', lambda: embed_case('embed'))
add('embed_positions', 'embed_positions', lambda: embed_case('bf16'))
add('embed_positions_f32', 'embed_positions_f32', lambda: embed_case('f32'))


def seq_case(kind):
    lengths = LENGTHS
    B, T = len(lengths), sum(lengths)
    if kind == 'positions':
        ops = [Operand('cu_lens', cu_of(lengths)), out('pos', (T,), I32), out('seq', (T,), I32)]

        def call(v):
            call_c('esme_hip_seq_positions', P(v['cu_lens']), B, T, P(v['pos']), P(v['seq']))
    else:
        ops = [Operand('cu_lens', cu_of(lengths)), out('order', (B,), I32)]

        def call(v):
            call_c('esme_hip_seq_order', P(v['cu_lens']), B, P(v['order']))
    return Case(f'seq_{kind}', ops, call)


add('seq_positions', 'seq_positions', lambda: seq_case('positions'))
add('seq_order', 'seq_order', lambda: seq_case('order'))


def gather_case(kind):
    R, E, n = 50, 320, 23
    if kind == 'gather':
        idx = torch.randint(0, R, (n,), generator=torch.Generator().manual_seed(1))
        idx[0], idx[1], idx[2], idx[3] = 0, R - 1, R, -1                   # the first and last rows; two indices outside [0, rows): zero rows
        ops = [Operand('src', rnd((R, E), 2), pad=False), Operand('idx', idx), out('dst', (n, E), pad=False)]

        def call(v):
            call_c('esme_hip_gather_rows', P(v['src']), R, P(v['idx']), P(v['dst']), n, E)
    else:
        idx = torch.cat((torch.tensor([0, R - 1, R, -1]), 1 + 2 * torch.arange(n - 4))).to(I64)        # distinct rows; two indices outside [0, rows): dropped
        ops = [Operand('src', rnd((n, E), 2), pad=False), Operand('idx', idx), Operand('dst', torch.zeros(R, E, dtype=BF), 'inout', pad=False)]

        def call(v):
            call_c('esme_hip_scatter_rows', P(v['src']), P(v['idx']), P(v['dst']), R, n, E)
    return Case(f'{kind}_rows', ops, call)


add('gather_rows', 'gather_rows', lambda: gather_case('gather'))
add('scatter_rows', 'scatter_rows', lambda: gather_case('scatter'))

POOL_LENGTHS = [0, 1, 65, 0, 129, 31, 0]       # empty sequences first, in the middle and last


def segment_mean_case(dt):
    B, T, E = len(POOL_LENGTHS), sum(POOL_LENGTHS), 320
    ops = [Operand('x', rnd((T, E), 1, dtype=dt)), Operand('cu_lens', cu_of(POOL_LENGTHS)), out('out', (B, E), dt)]

    def call(v):
        call_c('esme_hip_segment_mean', P(v['x']), v['x'].stride(0), P(v['cu_lens']), B, E, P(v['out']), v['out'].stride(0), int(dt == F32))
    return Case(f'segment_mean {dt}', ops, call)


add('segment_mean-bf16', 'segment_mean', lambda: segment_mean_case(BF))
add('segment_mean-f32', 'segment_mean', lambda: segment_mean_case(F32))


# ------------------------------------------------------------------ pooling, LoRA

def pool_case(kind, dt=BF):
    from esme import _hip
    E, heads, n_cls = 320, 20, 2
    B, T = len(POOL_LENGTHS), sum(POOL_LENGTHS)
    if kind == 'fold':
        ops = [Operand('cls', rnd((n_cls, E), 1)), Operand('w_k', rnd((E, E), 2, E ** -0.5)), out('U', (n_cls * heads, E), F32, pad=False)]

        def call(v):
            call_c('esme_hip_attn_pool_fold', P(v['cls']), v['cls'].stride(0), P(v['w_k']), v['w_k'].stride(0), E, heads, n_cls, P(v['U']))
    elif kind == 'pool':
        nbytes = _hip.attn_pool_workspace_bytes(B, T, E, heads, n_cls)
        assert nbytes == (B + T // 64 + 1) * (2 * n_cls * heads + n_cls * E) * 4          # the header's formula
        ops = [Operand('x', rnd((T, E), 1, dtype=dt)), Operand('cu_lens', cu_of(POOL_LENGTHS)), Operand('U', rnd((n_cls * heads, E), 3, 0.3, F32), pad=False),
               Operand('ws', torch.empty(nbytes, dtype=torch.uint8), 'ws'), out('out', (B, n_cls * E), dt)]

        def call(v):
            call_c('esme_hip_attn_pool', P(v['x']), v['x'].stride(0), P(v['cu_lens']), B, T, E, heads, n_cls, P(v['U']), P(v['ws']), nbytes, P(v['out']), v['out'].stride(0),
                   int(dt == F32))
    else:
        M, N, K = 37, 33, 320
        ops = [Operand('h', rnd((M, K), 1, dtype=dt)), Operand('w', rnd((N, K), 2, K ** -0.5)), Operand('bias', rnd((N,), 3)), out('y', (M, N), dt)]

        def call(v):
            call_c('esme_hip_relu_linear', P(v['h']), v['h'].stride(0), P(v['w']), v['w'].stride(0), P(v['bias']), P(v['y']), v['y'].stride(0), M, N, K, int(dt == F32))
    return Case(f'{kind} {dt}', ops, call)


add('attn_pool_fold', 'attn_pool_fold', lambda: pool_case('fold'))
for _dt, _n in ((BF, 'bf16'), (F32, 'f32')):
    add(f'attn_pool-{_n}', 'attn_pool', lambda dt=_dt: pool_case('pool', dt))
    add(f'relu_linear-{_n}', 'relu_linear', lambda dt=_dt: pool_case('relu', dt))


def lora_case(kind, T):
    E, X, rank = 320, 64, 24
    ops = [Operand('xu', torch.cat((rnd((T, E), 1), rnd((T, X), 2)), 1).contiguous(), 'inout'), Operand('A', rnd((rank, E), 3, E ** -0.5), pad=False)]
    if kind == 'ln':
        x = ops[0].data[:, :E].double()
        ops += [Operand('sums', torch.stack((x.sum(1), (x * x).sum(1)), 1).float(), pad=False), Operand('c1', rnd((rank,), 4, 1.0, F32)), Operand('bA', rnd((rank,), 5, 1.0, F32))]

    def call(v):
        xu = v['xu']
        args = [P(xu), xu.stride(0), P(v['A']), rank, T, E, X, P(xu) + 2 * E, xu.stride(0)]
        if kind == 'ln':
            call_c('esme_hip_lora_down_ln', *args, P(v['sums']), 1, E, 1e-5, P(v['c1']), P(v['bA']))
        else:
            call_c('esme_hip_lora_down', *args)
    return Case(f'lora_down {kind} T{T}', ops, call)


for _T in (1, 257):
    add(f'lora_down-T{_T}', 'lora_down', lambda T=_T: lora_case('plain', T))
    add(f'lora_down_ln-T{_T}', 'lora_down_ln', lambda T=_T: lora_case('ln', T))


# ------------------------------------------------------------------ quantisation

CODEBOOK = [-1.0, -0.6962, -0.5251, -0.3949, -0.2844, -0.1848, -0.0911, 0.0, 0.0796, 0.1609, 0.2461, 0.3379, 0.4407, 0.5626, 0.723, 1.0]


def quant_case(kind, N, K):
    cb = (ctypes.c_float * 16)(*CODEBOOK)
    g = torch.Generator().manual_seed(N + K)
    if kind == 'q4':
        ops = [Operand('w', rnd((N, K), 1)), out('codes', (N, K // 2), torch.uint8, pad=False), out('absmax', (N, K // 64), F32, pad=False)]

        def call(v):
            call_c('esme_hip_quantize_4bit', P(v['w']), v['w'].stride(0), N, K, cb, P(v['codes']), P(v['absmax']))
    elif kind == 'dq4':
        ops = [Operand('codes', torch.randint(0, 256, (N, K // 2), generator=g).to(torch.uint8), pad=False), Operand('absmax', torch.rand(N, K // 64, generator=g), pad=False),
               Operand('col_scale', 0.5 + torch.rand(K, generator=g)), out('out', (N, K))]

        def call(v):
            call_c('esme_hip_dequantize_4bit', P(v['codes']), P(v['absmax']), N, K, cb, P(v['col_scale']), P(v['out']), v['out'].stride(0))
    elif kind == 'q8':
        ops = [Operand('w', rnd((N, K), 1)), out('codes', (N, K), torch.int8, pad=False), out('scale', (N,), F32)]

        def call(v):
            call_c('esme_hip_quantize_8bit', P(v['w']), v['w'].stride(0), N, K, P(v['codes']), P(v['scale']))
    else:
        ops = [Operand('codes', torch.randint(-127, 128, (N, K), generator=g).to(torch.int8), pad=False), Operand('scale', torch.rand(N, generator=g)),
               Operand('col_scale', 0.5 + torch.rand(K, generator=g)), out('out', (N, K))]

        def call(v):
            call_c('esme_hip_dequantize_8bit', P(v['codes']), P(v['scale']), N, K, P(v['col_scale']), P(v['out']), v['out'].stride(0))
    return Case(f'{kind} {N}x{K}', ops, call)


for _N, _K in [(4, 64), (33, 64), (5, 320)]:          # N * K = 256 (one block of threads), 2112 and 1600 (off every power-of-two boundary)
    add(f'quantize_4bit-{_N}x{_K}', 'quantize_4bit', lambda N=_N, K=_K: quant_case('q4', N, K))
    add(f'dequantize_4bit-{_N}x{_K}', 'dequantize_4bit', lambda N=_N, K=_K: quant_case('dq4', N, K))
    add(f'quantize_8bit-{_N}x{_K}', 'quantize_8bit', lambda N=_N, K=_K: quant_case('q8', N, K))
    add(f'dequantize_8bit-{_N}x{_K}', 'dequantize_8bit', lambda N=_N, K=_K: quant_case('dq8', N, K))


# ------------------------------------------------------------------ the one-call forwards

FWD_LENGTHS = [33, 150, 70]                         # T = 253: the last row tile is ragged in every GEMM (128- and 256-row tiles)
_MODELS = {}


def _model(kind, L, E, H):
    key = (kind, L, E, H)
    if key not in _MODELS:
        from esme import ESM, synthetic as syn
        with tempfile.TemporaryDirectory() as td:
            path = syn.write_checkpoint(os.path.join(td, 'm.safetensors'), f'{kind}_test', L, E, H, seed=23)
            _MODELS[key] = ESM.from_pretrained(path, device=DEV)
    return _MODELS[key]


def forward_case(mode, kind, L, E, H):
    from esme import _hip, cforward, synthetic as syn
    model = _model(kind, L, E, H)
    model.set_precision({'fast': 'fast', 'half': 'half', 'exact': 'exact'}[mode])
    lib = _hip.load()
    tokens, cu, ml = syn.random_tokens(FWD_LENGTHS, seed=4).to(DEV), syn.cu_lens_of(FWD_LENGTHS).to(DEV), max(FWD_LENGTHS)
    T, Ep, B = tokens.numel(), model.phys_dim, len(FWD_LENGTHS)
    with _hip.stream_scope(DEV):
        x = model._embedding_phys(tokens, (cu, ml))
        ctx = model._context(cu, ml, T, x.device)
        x32 = model._embedding_exact(x, tokens, (cu, ml), None) if mode != 'fast' else None
    md = cforward.ModelDescriptor(model, f16=mode == 'half', plan=ctx.plan if mode == 'half' else None, exact=mode == 'exact')
    d = md.desc
    d.cos, d.sin, d.table_len = P(ctx.cos), P(ctx.sin), int(ctx.cos.shape[0]) if ctx.cos is not None else 0
    keep = [md, ctx, model]
    zero_pair = torch.zeros(T, 2 * Ep, dtype=BF)
    if mode == 'fast':
        lm = model.lm_head
        dw, db, fw = lm._padded_weights() if model.padded else (lm.dense.weight, lm.dense.bias, lm.final.weight)
        d.head_dense_w, d.head_dense_b, d.head_ln_w, d.head_ln_b = P(dw), P(db), P(lm.layer_norm.weight), P(lm.layer_norm.bias)
        d.head_final_w, d.head_final_b = P(fw), P(lm.final.bias)
        nbytes = int(lib.esme_hip_forward_workspace_bytes(ctypes.byref(d), T))
        ops = [Operand('x', x.cpu(), 'inout'), Operand('cu_lens', cu.cpu()), Operand('pos', ctx.pos.cpu()), Operand('ws', torch.empty(nbytes, dtype=torch.uint8), 'ws'),
               out('logits', (T, model.vocab_size))]

        def call(v):
            call_c('esme_hip_forward', ctypes.byref(d), P(v['x']), v['x'].stride(0), P(v['cu_lens']), B, T, ml, P(v['pos']), P(v['ws']), nbytes, P(v['logits']), v['logits'].stride(0))
    else:
        if mode == 'half':
            d.half_overflow_flag, d.cos32, d.sin32 = P(ctx.ovf), P(ctx.cos32), P(ctx.sin32)
            nbytes = int(lib.esme_hip_forward_half_workspace_bytes(ctypes.byref(d), T))
        else:
            nbytes = int(lib.esme_hip_forward_exact_workspace_bytes(ctypes.byref(d), T))
        # padded layouts: the pad columns of `pair` are left as they are ("pass zeros"): an inout operand of zeros; exact + padded: a ZEROED workspace (header)
        ops = [Operand('x32', x32.cpu(), 'inout' if mode == 'exact' else 'in'), Operand('cu_lens', cu.cpu()), Operand('pos', ctx.pos.cpu()),
               Operand('ws', torch.empty(nbytes, dtype=torch.uint8), 'ws', zeroed=mode == 'exact' and model.padded),
               Operand('pair', zero_pair, 'inout') if model.padded else out('pair', (T, 2 * Ep)),
               Operand('rep32', torch.zeros(T, Ep), 'inout') if model.padded else out('rep32', (T, Ep), F32)]

        def call(v):
            call_c('esme_hip_forward_half' if mode == 'half' else 'esme_hip_forward_exact', ctypes.byref(d), P(v['x32']), v['x32'].stride(0), P(v['cu_lens']), B, T, ml, P(v['pos']),
                   P(v['ws']), nbytes, P(v['pair']), v['pair'].stride(0), P(v['rep32']), v['rep32'].stride(0))
    case = Case(f'forward {mode} {kind} L{L} E{E}', ops, call)
    case.keep = keep
    return case


for _kind, _L, _E, _H in [('esm2', 2, 320, 20), ('esmc', 2, 960, 15), ('esm2', 2, 480, 20)]:
    add(f'forward-{_kind}-E{_E}', 'forward forward_workspace_bytes', lambda k=_kind, L=_L, E=_E, H=_H: forward_case('fast', k, L, E, H))
    add(f'forward_half-{_kind}-E{_E}', 'forward_half forward_half_workspace_bytes', lambda k=_kind, L=_L, E=_E, H=_H: forward_case('half', k, L, E, H))
    add(f'forward_exact-{_kind}-E{_E}', 'forward_exact forward_exact_workspace_bytes', lambda k=_kind, L=_L, E=_E, H=_H: forward_case('exact', k, L, E, H))


# ------------------------------------------------------------------ the test

@pytest.mark.parametrize('spec', CASES, ids=[c.id for c in CASES])
def test_footprint(spec, monkeypatch):
    from esme import _hip
    lib, called = _hip.load(), set()

    class Recorder:
        """The loaded library with every esme_hip_* call noted: the case must reach the entry points its coverage label names."""
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if not name.startswith('esme_hip_') or not callable(fn):
                return fn

            def wrapped(*a):
                called.add(name)
                return fn(*a)
            return wrapped
    monkeypatch.setattr(_hip, '_lib', Recorder())
    case = spec.build()                      # (builders call the size queries: esme_hip_*_workspace_bytes, esme_hip_gemm_stats_blocks_opts)
    res = fp.check(case, DEV)
    monkeypatch.undo()
    assert set(spec.symbols) <= called, f'{spec.id}: labelled {sorted(spec.symbols)}, but the run called {sorted(called)}'
    # the case itself is sound: every floating-point output holds finite values (bit-equal NaNs would pass the comparisons above)
    for op in case.operands:
        if op.role == 'out' and op.data.dtype.is_floating_point:
            assert bool(torch.isfinite(res['nan'].outputs[op.name].view(op.data.dtype).float()).all()), f'{case.name}: output {op.name} is not finite'
