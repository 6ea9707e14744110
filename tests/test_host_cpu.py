"""CPU-side tests (run with -m "not gpu"): the C-ABI library loads and exports every
symbol include/esme_hip.h declares, host-side logic (tokenizer shapes, synthetic
checkpoints, packing, loader, API errors, fail-loudly behaviour), and the N>1 sharding
path on the gloo backend with world_size 2.  No compute is launched on a GPU here."""
import ctypes
import os
import re
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_exported_and_bound():
    from esme import _hip
    header = open(os.path.join(ROOT, 'include', 'esme_hip.h')).read()
    declared = set(re.findall(r'\b(esme_hip_\w+)\s*\(', header))
    assert declared, 'no declarations parsed'
    lib = ctypes.CDLL(_hip.lib_path())
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/esme_hip.h but not exported'
    assert declared == set(_hip.SIGNATURES), declared ^ set(_hip.SIGNATURES)
    assert _hip.load().esme_hip_abi_version() == _hip.ABI_VERSION
    m = re.search(r'#define\s+ESME_HIP_ABI_VERSION\s+(\d+)', header)
    assert int(m.group(1)) == _hip.ABI_VERSION


def test_ctypes_structs_match_the_header_layout(tmp_path):
    """The Python binding restates five structs of include/esme_hip.h by hand; a field added on one side only would shift every
    later field silently.  gcc prints sizeof / offsetof of every field from the header itself; the ctypes mirrors must agree."""
    import shutil
    import subprocess
    from esme import _hip
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc in this environment')
    structs = {'esme_gemm_fusion_t': _hip.GemmFusion, 'esme_gemm_opts_t': _hip.GemmOpts, 'esme_attn_opts_t': _hip.AttnOpts,
               'esme_layer_weights_t': _hip.LayerWeights, 'esme_model_desc_t': _hip.ModelDesc}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "esme_hip.h")}"', 'int main(void) {']
    for cname, py in structs.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run([gcc, '-std=c99', '-o', str(exe), str(src)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    seen = 0
    for line in out.splitlines():
        cname, field, value = line.split()
        py = structs[cname]
        expect = ctypes.sizeof(py) if field == 'sizeof' else getattr(py, field).offset
        assert int(value) == expect, f'{cname}.{field}: header {value}, ctypes {expect}'
        seen += 1
    assert seen == sum(len(py._fields_) + 1 for py in structs.values())
    # and the header has no field the mirrors lack (same field count per struct)
    header = open(os.path.join(ROOT, 'include', 'esme_hip.h')).read()
    for cname, py in structs.items():
        end = header.index('} ' + cname + ';')
        start = header.rfind('typedef struct', 0, end)
        body = header[header.index('{', start) + 1:end]
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        n = sum(len(decl.split(',')) for decl in body.split(';') if decl.strip())
        assert n == len(py._fields_), f'{cname}: {n} fields in the header, {len(py._fields_)} in the ctypes mirror'


def test_argument_validation_without_gpu():
    """Host-side checks of the C entry points reject bad arguments before any launch."""
    from esme import _hip
    lib = _hip.load()
    assert lib.esme_hip_gemm_bf16(None, 64, None, None, None, 0, None, 64, 8, 64, 64, 0, 1.0, None) == -1
    assert b'null' in lib.esme_hip_last_error()
    assert lib.esme_hip_gemm_bf16(16, 100, 16, None, None, 0, 16, 64, 8, 64, 100, 0, 1.0, None) == -2
    assert b'multiple of 64' in lib.esme_hip_last_error()
    assert lib.esme_hip_gemm_bf16(16, 64, 16, None, None, 0, 16, 64, 8, 64, 64, 9, 1.0, None) == -1
    assert lib.esme_hip_attn_varlen_fwd(16, 16, 16, 64, 16, 64, 16, 1, 8, 1, 24, 8, 0.2, None) == -2
    assert b'head dim' in lib.esme_hip_last_error()
    assert lib.esme_hip_layernorm(16, 8, 16, None, 16, 8, 4, 12, 1e-5, None) == -1      # E % 8 != 0
    assert lib.esme_hip_rotary_varlen(16, 16, 64, 16, 16, 16, 4, 2, 24, 8, None) == -2   # d % 16 != 0
    assert lib.esme_hip_gemm_bf16(None, 0, None, None, None, 0, None, 0, 0, 64, 64, 0, 1.0, None) == 0   # M = 0: no-op


def test_round5_entry_points_validate_without_gpu():
    """The round-5 entries (precision 'half' made robust, the one-call 'exact' stack) reject bad arguments on the host, before any launch:
    runs without a GPU and under the host-side AddressSanitizer build (tools/asan_host_check.sh)."""
    from esme import _hip
    lib = _hip.load()
    # stream_operand_scaled: a scale / an extension tile belongs to the pair form; the tile sits between hi and lo
    assert lib.esme_hip_stream_operand_scaled(16, 64, 16, 64, 0, 1, 16, None, 0, 0, None, 4, 64, None) == -1
    assert b'pair form' in lib.esme_hip_last_error()
    assert lib.esme_hip_stream_operand_scaled(16, 64, 16, 192, 128, 1, None, 16, 4, 96, None, 4, 64, None) == -1      # ext_off + 64 > lo_off
    assert b'extension tile' in lib.esme_hip_last_error()
    assert lib.esme_hip_stream_operand_scaled(16, 64, 16, 192, 128, 1, None, None, 65, 64, None, 4, 64, None) == -1    # > 64 channels
    # q/k-pair attention: head dims 16 / 32 / 64, a positive lo offset
    assert lib.esme_hip_attn_varlen_fwd_qkpair_f16(16, 16, 16, 640, 384, 16, 128, 16, 1, 8, 1, 128, 8, 0.1, None, None) == -2
    assert b'head dim' in lib.esme_hip_last_error()
    assert lib.esme_hip_attn_varlen_fwd_qkpair_f16(16, 16, 16, 640, 0, 16, 128, 16, 1, 8, 2, 64, 8, 0.1, None, None) == -1
    # rotary on fp16 pairs: the lo block must not overlap the heads
    assert lib.esme_hip_rotary_split_f16(16, 256, 64, 16, 16, 16, 4, 2, 64, 8, None) == -1
    # the checked LayerNorm: same layout rules as esme_hip_layernorm_split
    assert lib.esme_hip_layernorm_split_checked(16, 128, 2, 32, 16, None, 16, 128, 64, None, 0, 4, 64, 1e-5, None, None) == -1
    # fused GEMM: pair scales / extension tile / overflow flag only where they belong
    fu = _hip.GemmFusion()
    fu.pair_scale_in = 16
    assert lib.esme_hip_gemm_bf16_fused(16, 64, 16, None, 16, 64, 16, 64, 8, 64, 64, 2, 1.0, ctypes.byref(fu), None) == -1
    assert b'pair stream' in lib.esme_hip_last_error()
    fu = _hip.GemmFusion()
    fu.pair_cols = 256
    assert lib.esme_hip_gemm_bf16_fused(16, 64, 16, None, None, 0, 16, 64, 8, 64, 64, 0, 1.0, ctypes.byref(fu), None) == -1
    fu = _hip.GemmFusion()
    fu.f16, fu.pair_off, fu.ext_off, fu.ext_n = 1, 128, 64, 65            # 65 channels in a 64-wide tile
    assert lib.esme_hip_gemm_bf16_fused(16, 64, 16, None, 16, 192, 16, 192, 8, 64, 64, 2, 1.0, ctypes.byref(fu), None) == -1
    assert b'extension tile' in lib.esme_hip_last_error()
    # whole-stack entries: descriptor of another ABI, workspace, head dim
    d = _hip.ModelDesc()
    assert lib.esme_hip_forward_exact_workspace_bytes(None, 8) == -1
    assert lib.esme_hip_forward_exact(ctypes.byref(d), 16, 64, 16, 1, 8, 8, 16, 16, 1 << 20, 16, 128, None, 0, None) == -1
    assert b'ABI' in lib.esme_hip_last_error()
    lw = (_hip.LayerWeights * 1)()
    d.struct_bytes, d.n_layers, d.embed_dim, d.phys_dim, d.heads, d.head_dim, d.head_pad, d.ffn_dim = ctypes.sizeof(_hip.ModelDesc), 1, 64, 64, 1, 48, 48, 256
    d.layers = lw
    need = lib.esme_hip_forward_exact_workspace_bytes(ctypes.byref(d), 8)
    assert need > 0
    assert lib.esme_hip_forward_exact(ctypes.byref(d), 16, 64, 16, 1, 8, 8, 16, 16, need, 16, 128, None, 0, None) == -2
    assert b'head dims' in lib.esme_hip_last_error()
    assert lib.esme_hip_forward_exact(ctypes.byref(d), 16, 64, 16, 1, 8, 8, 16, 16, need - 1, 16, 128, None, 0, None) == -1
    d.half_ext_n = 65
    assert lib.esme_hip_forward_half(ctypes.byref(d), 16, 64, 16, 1, 8, 8, 16, 16, 1 << 24, 16, 128, None, 0, None) == -1
    assert b'half_ext_n' in lib.esme_hip_last_error()


def test_round6_entry_points_validate_without_gpu():
    """The round-6 entries (the plan guard of precision 'half', per-call options of the q/k-pair attention) reject bad arguments on the host, before any launch."""
    from esme import _hip
    lib = _hip.load()
    # guarded stream operand: the column maxima belong to the pair form and must be 16-byte aligned
    assert lib.esme_hip_stream_operand_guarded(16, 64, 16, 64, 0, 1, None, None, 0, 0, None, 16, 4, 64, None) == -1
    assert b'col_absmax' in lib.esme_hip_last_error()
    assert lib.esme_hip_stream_operand_guarded(16, 64, 16, 128, 64, 1, None, None, 0, 0, None, 20, 4, 64, None) == -1       # misaligned
    # fused GEMM: col_absmax only on the fp16 pair stream's residual epilogue, qk_sumsq only on the fp16 LN-folded projection with fused rotary
    fu = _hip.GemmFusion()
    fu.col_absmax = 16
    assert lib.esme_hip_gemm_bf16_fused(16, 64, 16, None, 16, 64, 16, 64, 8, 64, 64, 2, 1.0, ctypes.byref(fu), None) == -1
    assert b'col_absmax' in lib.esme_hip_last_error()
    fu = _hip.GemmFusion()
    fu.qk_sumsq, fu.f16 = 16, 1
    assert lib.esme_hip_gemm_bf16_fused(16, 64, 16, None, None, 0, 16, 64, 8, 64, 64, 0, 1.0, ctypes.byref(fu), None) == -1
    assert b'qk_sumsq' in lib.esme_hip_last_error()
    # q/k-pair attention with options: a struct of another ABI is refused; head dim 128 has no pair form
    ao = _hip.AttnOpts(4, 0, 0, 0.0, 0, None, 0, 1)
    assert lib.esme_hip_attn_varlen_fwd_qkpair_f16_opts(16, 16, 16, 640, 384, 16, 128, 16, 1, 8, 2, 64, 8, 0.1, ctypes.byref(ao), None) == -1
    assert b'ABI' in lib.esme_hip_last_error()
    ao = _hip.AttnOpts(ctypes.sizeof(_hip.AttnOpts), 2, 0, 0.0, 0, None, 0, 1)
    assert lib.esme_hip_attn_varlen_fwd_qkpair_f16_opts(16, 16, 16, 640, 384, 16, 128, 16, 1, 8, 1, 128, 8, 0.1, ctypes.byref(ao), None) == -2
    # guarded q/k pass: alignment of the maxima
    assert lib.esme_hip_qk_norm_rotary_f16_guarded(16, 16, 128, 16, 16, None, None, 1e-5, 16, 16, 16, 4, 2, 64, 8, 18, None) == -1
    assert b'qk_sumsq' in lib.esme_hip_last_error()
    # the same with the softmax scale folded into q (ABI 10: the fixed-reference form of the fp16 attention kernel): the scale must be a positive number
    assert lib.esme_hip_qk_norm_rotary_f16_scaled(16, 16, 128, 16, 16, None, None, 1e-5, 16, 16, 16, 4, 2, 64, 8, 0.18, 18, None) == -1
    assert b'qk_sumsq' in lib.esme_hip_last_error()
    for bad in (0.0, -1.0, float('nan')):
        assert lib.esme_hip_qk_norm_rotary_f16_scaled(16, 16, 128, 16, 16, None, None, 1e-5, 16, 16, 16, 4, 2, 64, 8, bad, None, None) == -1
        assert b'q_scale' in lib.esme_hip_last_error()
    assert lib.esme_hip_qk_norm_rotary_f16_scaled(16, 16, 128, 16, 16, None, None, 1e-5, 16, 16, 16, 0, 2, 64, 8, 0.18, None, None) == 0       # T = 0: nothing to do
    # fp16 attention with q_prescaled: the fixed-reference form exists for head dims 64 / 32 only
    cu_dummy = 16
    ao = _hip.AttnOpts(ctypes.sizeof(_hip.AttnOpts), 0, 0, 8.0, 1, None, 1, 1)
    assert lib.esme_hip_attn_varlen_fwd_opts(16, 16, 16, 128, 16, 128, cu_dummy, 1, 32, 1, 128, 32, 0.125, ctypes.byref(ao), None) == -1
    assert b'q_prescaled' in lib.esme_hip_last_error()


def test_attention_generic_kernel_limits_validate_without_gpu():
    """The generic and split attention kernels address rows inside one sequence with 32-bit element offsets and take the sequence from
    grid z (more than 65 535 sequences run as several launches that advance cu_lens).  Refused on the host, before any launch: a row stride
    for which (max_len + the kernel's row tile) rows reach 2^32 elements, and a dispatch order with more than 65 535 sequences.  Every call
    here is refused; that B = 70 000 is accepted is shown by tests/test_extreme_shapes_gpu.py."""
    from esme import _hip
    lib = _hip.load()
    cu = 16
    # (128 + 128 rows) * 2^24 = 2^32 elements: the first refused stride (max_len < 192: one 128-row q-block per wave)
    ld = 1 << 24
    for d, variant in ((16, 0), (128, 0), (64, 0), (32, 0), (64, 1), (64, 2)):        # head dims 64 / 32: fits32 fails, so the generic kernel
        ao = _hip.AttnOpts(ctypes.sizeof(_hip.AttnOpts), variant, 0, 8.0, 1, None, 0, 0)
        assert lib.esme_hip_attn_varlen_fwd_opts(16, 16, 16, ld, 16, 128, cu, 1, 8, 1, d, 128, 0.25, ctypes.byref(ao), None) == -2, (d, variant)
        assert b'2^32' in lib.esme_hip_last_error()
    assert lib.esme_hip_attn_varlen_fwd(16, 16, 16, ld, 16, 128, cu, 1, 8, 1, 16, 128, 0.25, None) == -2
    assert lib.esme_hip_attn_varlen_fwd_exact(16, 16, 16, ld, 16, 128, cu, 1, 8, 1, 128, 128, 0.25, None) == -2
    # max_len >= 192: two q-blocks per wave, a 256-row tile: (64 + 192) rows at 2^24 already reach 2^32
    assert lib.esme_hip_attn_varlen_fwd(16, 16, 16, ld, 16, 128, cu, 1, 8, 1, 16, 192, 0.25, None) == -2
    assert b'max_len + 256' in lib.esme_hip_last_error()
    # the split ('exact') and q/k-pair ('half', robust) entries: 128-row tiles
    for d in (16, 32, 64, 128):
        assert lib.esme_hip_attn_varlen_fwd_split(16, 16, 16, ld, 64, 16, 512, 256, cu, 1, 8, 1, d, 128, 0.25, None, None) == -2, d
        assert b'attn_split' in lib.esme_hip_last_error() and b'2^32' in lib.esme_hip_last_error()
    for d in (16, 32, 64):
        assert lib.esme_hip_attn_varlen_fwd_qkpair_f16(16, 16, 16, ld, 64, 16, 128, cu, 1, 8, 1, d, 128, 0.25, None, None) == -2, d
        assert b'attn_qkpair' in lib.esme_hip_last_error() and b'2^32' in lib.esme_hip_last_error()
    # a dispatch order with more than 65 535 sequences: the chunked launches advance cu_lens, an order into the whole batch would mis-index
    B = 70000
    for d, variant in ((16, 0), (128, 0), (64, 1), (32, 1)):
        ao = _hip.AttnOpts(ctypes.sizeof(_hip.AttnOpts), variant, 0, 8.0, 1, 16, 0, 0)
        assert lib.esme_hip_attn_varlen_fwd_opts(16, 16, 16, 128, 16, 128, cu, B, B, 1, d, 8, 0.25, ctypes.byref(ao), None) == -1, (d, variant)
        assert b'seq_order' in lib.esme_hip_last_error()
    for d in (16, 64):
        assert lib.esme_hip_attn_varlen_fwd_split(16, 16, 16, 384, 192, 16, 128, 64, cu, B, B, 1, d, 8, 0.25, 16, None) == -1, d
        assert b'seq_order' in lib.esme_hip_last_error()
        assert lib.esme_hip_attn_varlen_fwd_qkpair_f16(16, 16, 16, 320, 192, 16, 64, cu, B, B, 1, d, 8, 0.25, 16, None) == -1, d
        assert b'seq_order' in lib.esme_hip_last_error()
    # the bounds that stay: H <= 65 535
    assert lib.esme_hip_attn_varlen_fwd(16, 16, 16, 65536 * 16, 16, 65536 * 16, cu, 1, 8, 65536, 16, 8, 0.25, None) == -1
    assert b'H <= 65535' in lib.esme_hip_last_error()


def test_calibration_batch_covers_the_vocabulary_and_plan_keys():
    """precision 'half' (round 6), host side: the calibration batch holds every id of the alphabet except <pad> at least 8 times, cls / eos at the ends of
    its 8 sequences, is the same on every machine, and takes a caller's batch on board; HalfPlan keys derived weights on the channel LIST."""
    import torch
    from esme.esm import ESM2, ESMC
    from esme import halfmode
    from esme.attention import HalfPlan, _ext_key
    for cls in (ESM2, ESMC):
        m = cls(num_layers=1, embed_dim=64, attention_heads=4)
        tok, cu, max_len = halfmode.calibration_batch(m)
        tok2, _, _ = halfmode.calibration_batch(m)
        assert torch.equal(tok, tok2) and tok.numel() == 1024 and cu.tolist()[0] == 0 and cu.tolist()[-1] == 1024 and max_len == 192
        counts = torch.bincount(tok, minlength=33)
        al = m.alphabet
        for i in range(len(al.alphabet)):
            if i == al.padding_idx:
                assert counts[i] == 0
            else:
                assert counts[i] >= 8, (cls.__name__, i, int(counts[i]))
        starts = cu[:-1].long()
        assert (tok[starts] == al.cls_idx).all() and (tok[cu[1:].long() - 1] == al.eos_idx).all()
        m.HALF_CALIB_VOCAB = 'residues'
        tr, _, _ = halfmode.calibration_batch(m)
        assert set(tr.tolist()) <= set(range(4, 24)) | {al.cls_idx, al.eos_idx}
        m.HALF_CALIB_VOCAB = 'all'
        m.set_precision('half', calib=(torch.tensor([0, 5, 24, 2, 0, 7, 2]), (torch.tensor([0, 4, 7], dtype=torch.int32), 4)))
        tu, cuu, ml = halfmode.calibration_batch(m)
        assert tu.numel() == 1031 and cuu.tolist()[-3:] == [1024, 1028, 1031] and tu[-7:].tolist() == [0, 5, 24, 2, 0, 7, 2]
    a, b = torch.tensor([3, 9], dtype=torch.int32), torch.tensor([3, 10], dtype=torch.int32)
    pa, pb = HalfPlan(a), HalfPlan(b)
    assert pa.ext_key == (3, 9) and _ext_key(a) == (3, 9) and _ext_key(b) == (3, 10) and pa.ext == 64 and HalfPlan().ext == 0
    assert _ext_key(torch.tensor([1, 2], dtype=torch.int32)) == (1, 2)
    # the fixed-reference attention form is a plan attribute (off unless a calibration switched it on), survives in describe(), and the switches exist
    assert not HalfPlan().qp and HalfPlan(qp=True).qp and 'fixed-reference' in HalfPlan(qp=True).describe() and 'fixed-reference' not in pa.describe()
    assert ESM2.HALF_QP_BOUND < ESM2.HALF_SCORE_BOUND and isinstance(ESM2.half_qp, bool)
    m = ESM2(num_layers=2, embed_dim=64, attention_heads=4)
    m.half_mode.plan = HalfPlan(qp=True, info={'calibrated': True}, qk_layers=[False, False])
    m.precision = 'half'
    vec = torch.zeros(1 + 64 + 2 + 2)
    vec[0], vec[1 + 3], vec[1 + 64 + 2:] = 1.0, 50.0, 1.0            # a stale verdict: channel 3 at 50 x the median
    with pytest.warns(RuntimeWarning):
        v = halfmode.plan_verdict(m, vec, update=True)
    assert v['updated'] and m.half_mode.plan.qp and m.half_mode.plan.ext_key == (3,)         # widening the plan keeps the attention form


def test_no_cpu_fallback_and_missing_library(monkeypatch):
    from esme import _hip, ESM2
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _hip.layernorm(x, torch.ones(64, dtype=torch.bfloat16))
    model = ESM2(num_layers=1, embed_dim=64, attention_heads=4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        model(torch.zeros(5, dtype=torch.int64), (torch.tensor([0, 5], dtype=torch.int32), 5))
    monkeypatch.setattr(_hip, '_lib', None)
    monkeypatch.setattr(_hip, '_LIB_PATH', '/nonexistent/libesme_hip.so')
    with pytest.raises(_hip.HipLibraryError, match='no CPU/torch fallback'):
        _hip.load()


def test_checkpoint_roundtrip_and_dispatch():
    from esme import ESM, ESM2, ESMC, synthetic as syn
    with tempfile.TemporaryDirectory() as td:
        p = syn.write_checkpoint(os.path.join(td, 'a.safetensors'), 'esm2_tiny', 2, 64, 4, seed=3)
        m = ESM.from_pretrained(p)
        assert isinstance(m, ESM2) and not isinstance(m, ESMC)
        sd, ref = m.state_dict(), syn.synthetic_state_dict('esm2', 2, 64, 3)
        assert list(sd) == list(ref) or set(sd) == set(ref)
        assert all(torch.equal(sd[k], ref[k]) for k in ref)
        assert all(v.dtype == torch.bfloat16 for v in sd.values())
        p = syn.write_checkpoint(os.path.join(td, 'c.safetensors'), 'esmc_tiny', 2, 128, 2, seed=4)
        m = ESM.from_pretrained(p)
        assert isinstance(m, ESMC) and m.lm_head.final.weight.shape == (64, 128)
        assert m.layers[0].residue_scaling == pytest.approx((2 / 36) ** 0.5)
        assert m.layers[0].final[1].activation.weight.shape == (512, 128)       # 8/3*128 -> 512
        with pytest.raises(AssertionError):
            ESM2.from_pretrained(p)                       # esmc weights into an ESM2
        with pytest.raises(AssertionError):
            ESM2.from_pretrained(p, quantization='2bit')
        with pytest.raises(AssertionError):
            ESM.from_pretrained(os.path.join(td, 'a.safetensors'), quantization='4bit', device='cpu')
    with pytest.raises(ValueError):
        ESM.from_pretrained('esm2_8m')                    # hub names need a download: out of scope


def test_qkv_packing_keeps_state_dict():
    from esme import ESM2
    torch.manual_seed(0)
    m = ESM2(num_layers=1, embed_dim=64, attention_heads=4)
    att = m.layers[0].self_attn
    before = {k: v.clone() for k, v in m.state_dict().items()}
    qkv_w = att._pack()[0]
    after = m.state_dict()
    assert set(before) == set(after) and all(torch.equal(before[k], after[k]) for k in before)
    assert qkv_w.shape == (192, 64) and att.q.weight.data_ptr() == qkv_w.data_ptr()
    assert att.k.weight.data_ptr() == qkv_w[64:].data_ptr()
    key = att._derived.key('pack')
    assert key is not None
    assert att._pack()[0] is qkv_w and att._derived.key('pack') == key      # idempotent


def test_synthetic_batches_and_flops():
    from esme import synthetic as syn
    tok, cu, ml, lens = syn.uniform_batch(50000, 500, seed=0)
    assert tok.numel() == 50000 and len(lens) == 100 and ml == 500 and cu[-1] == 50000
    assert int(tok[0]) == 0 and int(tok[499]) == 2 and tok[1:499].min() >= 4 and tok.max() <= 23
    lens = syn.proteome_lengths(50000, seed=0)
    assert sum(lens) == 50000 and min(lens) >= 3 and max(lens) <= 3502
    assert lens == syn.proteome_lengths(50000, seed=0)
    f = syn.algorithmic_flops('esm2', 33, 1280, [500] * 100)
    assert abs(f / 50000 / 1e6 - 1385.45) < 0.01           # 1 385.45 MFLOP / residue
    assert syn.swiglu_width(1152) == 3072 and syn.swiglu_width(960) == 2560


def test_partition_is_balanced_and_complete():
    from esme import shard, synthetic as syn
    lens = syn.proteome_lengths(50000, seed=3)
    for world in (1, 2, 3, 8):
        plan = shard.partition_sequences(lens, world)
        assert sorted(i for p in plan for i in p) == list(range(len(lens)))
        loads = [sum(lens[i] for i in p) for p in plan]
        assert max(loads) - min(loads) <= max(lens)
    assert shard.partition_sequences([5, 5], 4) == [[0], [1], [], []]


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, lengths, out_path, dtype=torch.bfloat16, pass_spec=True):
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(ROOT, 'esm-efficient_amd'))
    from esme import shard, synthetic as syn
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    tokens, cu = syn.random_tokens(lengths, seed=1), syn.cu_lens_of(lengths)
    table = torch.arange(33 * 8, dtype=torch.float32).view(33, 8).to(torch.bfloat16)

    def fake_forward(tok, pad_args):
        cu_r, max_len = pad_args
        assert tok.numel() == int(cu_r[-1]) and max_len == int((cu_r[1:] - cu_r[:-1]).max())
        pos = torch.arange(tok.numel()) - torch.repeat_interleave(cu_r[:-1].long(), (cu_r[1:] - cu_r[:-1]).long())
        out = table[tok].clone()
        out[:, 0] = pos.to(torch.bfloat16)             # position inside its own sequence
        return out.to(dtype)

    if pass_spec:
        full = shard.sharded_forward(fake_forward, tokens, cu, 'cpu', out_width=8, out_dtype=dtype)     # (known locally: no second collective)
    else:
        full = shard.sharded_forward(fake_forward, tokens, cu, 'cpu')      # an arbitrary callable: the idle rank learns width / dtype from one tiny all-reduce
    if rank == 0:
        torch.save(full, out_path)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('lengths', [[7, 3, 12, 5, 9], [4], [6, 6, 6]])
def test_sharded_forward_gloo_world2(lengths):
    """N>1 path on CPU: 2 ranks, gloo.  The gathered result must equal the single-rank
    result in input order (rows carry their token id and in-sequence position)."""
    from esme import synthetic as syn
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, 'full.pt')
        mp.spawn(_worker, args=(2, _free_port(), lengths, out), nprocs=2, join=True)
        full = torch.load(out)
    tokens, cu = syn.random_tokens(lengths, seed=1), syn.cu_lens_of(lengths)
    table = torch.arange(33 * 8, dtype=torch.float32).view(33, 8).to(torch.bfloat16)
    ref = table[tokens].clone()
    pos = torch.arange(tokens.numel()) - torch.repeat_interleave(cu[:-1].long(), (cu[1:] - cu[:-1]).long())
    ref[:, 0] = pos.to(torch.bfloat16)
    assert torch.equal(full, ref)


def test_sharded_forward_gloo_world2_fp32_logits_and_an_empty_rank():
    """precision='exact' returns fp32 logits: the gather keeps the dtype, and a rank that received no sequence (one sequence, two
    ranks) contributes an empty fp32 block of the right width -- both known locally (the model's vocab_size / precision, or the arguments),
    not learned through a second collective."""
    from esme import synthetic as syn
    lengths = [11]
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, 'full.pt')
        mp.spawn(_worker, args=(2, _free_port(), lengths, out, torch.float32), nprocs=2, join=True)
        full = torch.load(out)
    tokens, cu = syn.random_tokens(lengths, seed=1), syn.cu_lens_of(lengths)
    table = torch.arange(33 * 8, dtype=torch.float32).view(33, 8).to(torch.bfloat16)
    ref = table[tokens].clone()
    ref[:, 0] = torch.arange(11).to(torch.bfloat16)
    assert full.dtype == torch.float32 and torch.equal(full, ref.float())


def test_sharded_forward_gloo_world2_unknown_callable_and_an_empty_rank():
    """`forward` is an arbitrary callable (think model.forward_representation: rows are embed_dim wide, not vocab_size) and one
    rank is idle.  The idle rank must not GUESS a logits-shaped block (mismatched all_gather sizes hang): without out_width / out_dtype the
    ranks agree on the row shape with one small all-reduce."""
    from esme import synthetic as syn
    lengths = [9]
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, 'full.pt')
        mp.spawn(_worker, args=(2, _free_port(), lengths, out, torch.float32, False), nprocs=2, join=True)
        full = torch.load(out)
    assert full.dtype == torch.float32 and full.shape == (9, 8)


def test_output_spec_is_only_inferred_for_logit_methods():
    from esme import shard

    class FakeModel:
        vocab_size, precision = 33, 'half'
        def forward(self, *a): ...
        def predict_log_prob(self, *a): ...
        def forward_representation(self, *a): ...
        __call__ = forward

    m = FakeModel()
    assert shard._output_spec(m, None, None) == (33, torch.float32)
    assert shard._output_spec(m.forward, None, None) == (33, torch.float32)
    assert shard._output_spec(m.predict_log_prob, None, None) == (33, torch.float32)
    m.precision = 'fast'
    assert shard._output_spec(m.predict_log_prob, None, None) == (33, torch.bfloat16)
    assert shard._output_spec(m.forward_representation, None, None) is None          # embed_dim-wide rows: not guessed
    assert shard._output_spec(lambda t, p: None, None, None) is None
    assert shard._output_spec(m.forward_representation, 1280, torch.bfloat16) == (1280, torch.bfloat16)


def test_feedforward_head_module():
    from esme.layer import FeedForward
    ff = FeedForward(16, 32)
    assert ff(torch.randn(5, 16)).shape == (5, 1)
    assert [n for n, _ in ff.named_parameters()] == ['linear1.weight', 'linear1.bias', 'linear2.weight', 'linear2.bias']


def test_feedforward_matches_reference_golden():
    """values pinned on the reference's own class (reference esme/layer.py:4-23;
    fixture tests/golden/make_golden_a16.py): its state dict loads strictly and the fp32 outputs agree."""
    from golden_util import load_golden
    from esme.layer import FeedForward
    g = load_golden('g12_feedforward.npz')
    ff = FeedForward(g['embed_dim'], g['hidden_dim'])
    sd = {k.replace('__', '.'): v for k, v in g.items() if '__' in k}
    ff.load_state_dict(sd, strict=True)
    assert all(p.dtype == torch.float32 for p in ff.parameters())          # fp32 default dtype like the reference
    with torch.no_grad():
        y = ff(g['x'])
    assert y.shape == g['y'].shape == (3, 7, 1)
    torch.testing.assert_close(y, g['y'], rtol=1e-6, atol=1e-6)


def _run_bench(args, env_extra=None, timeout=300):
    import subprocess
    env = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, capture_output=True, text=True,
                          timeout=timeout, cwd=ROOT, env=env)


def test_bench_refuses_world_size_mismatch():
    """A launcher world size that differs from --gpus must be an error, never a mislabelled 1-GPU line."""
    out = _run_bench(['--gpus', '2', '--steps', '1', '--warmup', '0'], {'RANK': '0', 'LOCAL_RANK': '0', 'WORLD_SIZE': '1'})
    assert out.returncode != 0 and 'WORLD_SIZE=1' in out.stderr and '{' not in out.stdout


def test_bench_refuses_zero_steps_and_dump_in_dry_run():
    """--steps is the number of timed steps that ms_per_step divides by: 0 is refused, not a division by zero after the run.  A dry run
    computes nothing, so there is nothing for --dump-outputs to write."""
    out = _run_bench(['--steps', '0'])
    assert out.returncode != 0 and 'must be at least 1' in out.stderr and '{' not in out.stdout
    out = _run_bench(['--gpus', '2', '--dry-run', '--dump-outputs', 'unused'])
    assert out.returncode != 0 and '--dump-outputs needs a real run' in out.stderr and '{' not in out.stdout


def test_bench_dump_outputs_whole_or_seeded_row_sample(tmp_path):
    """bench.dump_outputs: float32 values of the whole array when it fits the budget; above it, the same rows on every call (a seeded
    sample, in row order), inside the budget."""
    import bench
    y = torch.randn(1000, 33, generator=torch.Generator().manual_seed(0)).bfloat16()
    note = bench.dump_outputs(str(tmp_path / 'whole'), 'logits', y, 1 << 20)
    a = np.load(tmp_path / 'whole' / 'logits.npy')
    assert note['rows'] == 'all' and a.dtype == np.float32 and np.array_equal(a, y.float().numpy())
    budget = 100 * 4 * 33
    notes = [bench.dump_outputs(str(tmp_path / d), 'logits', y, budget) for d in ('a', 'b')]
    a, b = np.load(tmp_path / 'a' / 'logits.npy'), np.load(tmp_path / 'b' / 'logits.npy')
    assert notes[0]['rows'] == '100 of 1000 (seeded sample)' and a.shape == (100, 33) and np.array_equal(a, b)
    assert a.nbytes <= budget
    full = y.float().numpy()
    idx = [int(np.flatnonzero((full == r).all(axis=1))[0]) for r in a]
    assert idx == sorted(set(idx)) and len(idx) == 100


@pytest.mark.skipif(torch.cuda.is_available(), reason='GPU boxes cover the self-launch path with RCCL (test_bench_contract_gpu.py)')
def test_bench_self_launches_n_ranks_without_a_launcher():
    """`python bench.py --gpus 2` with no RANK in the environment re-executes itself under torch.distributed.run
    with 2 ranks.  There is no HIP device here, so each rank stops at the device-count check -- which proves that
    two ranks were started with WORLD_SIZE=2 (the round-1 bug: it silently ran one rank and printed n_gpus 1)."""
    out = _run_bench(['--gpus', '2', '--steps', '1', '--warmup', '0'], timeout=600)
    assert out.returncode != 0 and '{' not in out.stdout
    # every rank prints the message unless the launcher's SIGTERM (sent when the first rank exits) reaches it first: what
    # must hold is that the device-count check fired and that a SECOND rank existed (its own message, or its entry in
    # torch.distributed.run's failure report)
    n = out.stderr.count('--gpus 2 but only 0 HIP devices are visible')
    assert n >= 1 and (n == 2 or 'local_rank: 1' in out.stderr), out.stderr[-3000:]


def test_bench_two_rank_dry_run_fields():
    """`bench.py --gpus 2 --dry-run`: the N > 1 bookkeeping end to end on CPU (gloo; no kernel runs, the line is marked
    dry_run and carries no value): self-launch with 2 ranks, fences, max-over-ranks step time with the per-rank spread, the
    logits all-gather timed SEPARATELY from the step, the world size the process group reports."""
    import json
    out = _run_bench(['--gpus', '2', '--dry-run', '--steps', '3', '--warmup', '1', '--model', 'esm2_8m', '--tokens', '1024',
                      '--seq-len', '256'], timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip().startswith('{')]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d['dry_run'] is True and d['value'] is None and d['n_gpus'] == 2 and d['steps'] == 3
    m = d['multi_gpu']
    assert m['world_size_seen'] == 2 and m['backend'] == 'gloo'
    assert 0 < m['rank_ms_per_step']['min'] <= m['rank_ms_per_step']['max'] and abs(m['rank_ms_per_step']['max'] - d['ms_per_step']) < 1e-3
    assert m['gather_ms'] > 0 and m['gather_bytes_per_rank'] == 1024 * 33 * 2
    assert abs(m['ms_per_step_incl_gather'] - (d['ms_per_step'] + m['gather_ms'])) < 2e-3


def test_gelu_polynomial_all_bf16_inputs():
    """The GEMM epilogue's GELU (csrc/common.h: gelu(x) = max(x, 0) - |x| 2^p(|x|), p a minimax polynomial of log2 Phi(-z))
    restated in numpy with the kernel's fp32 arithmetic (coefficients parsed from the header, fused multiply-adds) and
    checked against float64 x Phi(x) over ALL finite bf16 inputs: error <= 1/2 bf16 ulp of the result, with an absolute floor
    of 1.5e-7 |x| (what torch's own fp32 0.5 x (1 + erf(x / sqrt 2)) resolves: it cancels catastrophically below x = -4).
    Replaces the reference's nn.GELU() (esme/attention.py:233, esme/head.py:26)."""
    from scipy.special import ndtr
    src = open(os.path.join(os.path.dirname(__file__), '..', 'esm-efficient_amd', 'csrc', 'common.h')).read()
    body = src[src.index('float gelu_poly(const float z)'):]
    body = body[:body.index('template <int DEG = ESME_GELU_DEG>')]
    deg7, deg5 = body.split('} else {')
    default = int(re.search(r'#define ESME_GELU_DEG (\d)', src).group(1))
    assert default in (5, 7)
    bits = (np.arange(65536, dtype=np.uint32) << 16)
    x = bits.view(np.float32)
    x = x[np.isfinite(x)]
    xd = x.astype(np.float64)
    ref = xd * ndtr(xd)
    half_ulp = 0.5 * 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref), 1e-300))) - 7)
    tol = np.maximum(half_ulp, 1.5e-7 * np.abs(xd))
    worst = {}
    for name, text, deg in (('7', deg7, 7), ('5', deg5, 5)):
        co = [float(v) for v in re.findall(r'(-?\d\.\d+(?:e-?\d+)?)f', text)]
        assert len(co) == deg + 1, (name, co)
        z = np.minimum(np.abs(x), np.float32(64.0))                 # the kernel clamps z: gelu(+inf) = +inf, not NaN
        f32 = lambda v: v.astype(np.float32)
        with np.errstate(over='ignore', invalid='ignore'):
            p = f32(z.astype(np.float64) * np.float64(np.float32(co[0])) + np.float64(np.float32(co[1])))   # fmaf: exact product, one rounding
            for c in co[2:]:
                p = f32(z.astype(np.float64) * p.astype(np.float64) + np.float64(np.float32(c)))
            e = f32(np.exp2(p.astype(np.float64)))
            y = f32(-(z.astype(np.float64)) * e.astype(np.float64) + np.maximum(x, 0).astype(np.float64))
        err = np.abs(y.astype(np.float64) - ref) / tol
        worst[name] = float(err.max())
        assert np.isfinite(y).all()
        # beyond the fitted range the polynomial must stay far below 0 up to the clamp, so that 2^p underflows to the limit
        zz = np.linspace(6.0, 64.0, 5801)
        pp = np.polyval(co, zz)
        assert pp.max() <= -29.0, (name, pp.max())
        # x = +-inf: z = 64, 2^p(64) = 0 exactly -> gelu(+inf) = +inf, gelu(-inf) = -64 * 0 + 0 = -0
        assert np.exp2(np.float32(np.polyval(co, 64.0))) == 0.0
    assert worst['7'] <= 0.01 and worst['5'] <= 0.25, worst          # fractions of (1/2 ulp | floor); the shipped degree is
    assert worst[str(default)] <= 0.25                                # far inside the 1/2-ulp bar


@pytest.mark.parametrize('d', [16, 32, 64])
def test_rotary_tables_bit_equal_reference(d):
    """RotaryEmbedding.tables() (the PRODUCT's host-side table builder) against the reference's cached tables
    (esme/rotary.py:116-149; golden g5_rotary.npz made by tests/golden/make_golden.py from RotaryEmbedding._cos_cached /
    _sin_cached): fp32 tables equal, bf16 tables bit for bit."""
    from golden_util import load_golden
    from esme.rotary import RotaryEmbedding
    g = load_golden('g5_rotary.npz')
    for dtype, tag in ((torch.float32, 'f32'), (torch.bfloat16, 'bf16')):
        cos, sin = RotaryEmbedding(d).tables(180, 'cpu', dtype)
        assert cos.shape == (180, d) and cos.dtype == dtype
        assert torch.equal(cos.float(), g[f'cos_d{d}_{tag}'].float()) and torch.equal(sin.float(), g[f'sin_d{d}_{tag}'].float())
    # a longer request regrows the cache and keeps the prefix
    rot = RotaryEmbedding(d)
    c1, _ = rot.tables(60, 'cpu', torch.bfloat16)
    c2, _ = rot.tables(180, 'cpu', torch.bfloat16)
    assert torch.equal(c2[:60], c1) and torch.equal(c2.float(), g[f'cos_d{d}_bf16'].float())


def test_descriptor_signature_sees_replaced_and_rewritten_parameters():
    """esme.cforward.ModelDescriptor.signature (what decides whether the C entry's cached descriptor -- raw pointers to derived
    weight copies -- is still valid) is O(1) in Python work per forward, yet must move when (a) a parameter OBJECT is replaced
    (the old cached parameter list kept the dead object alive and never noticed), (b) a parameter is rewritten in
    place, (c) load_state_dict / invalidate_graphs run; and must NOT move otherwise."""
    from esme.cforward import ModelDescriptor
    from esme.esm import ESM2
    m = ESM2(num_layers=2, embed_dim=64, attention_heads=4)
    s0 = ModelDescriptor.signature(m)
    assert ModelDescriptor.signature(m) == s0
    lin = m.layers[1].self_attn.out
    lin.weight = torch.nn.Parameter(torch.zeros_like(lin.weight), requires_grad=False)          # (a)
    s1 = ModelDescriptor.signature(m)
    assert s1 != s0
    assert any(p is lin.weight for p in m.__dict__['_cparams'][1])                                 # the cached list follows the new object
    with torch.no_grad():
        m.layers[0].final[1].weight.copy_(torch.ones_like(m.layers[0].final[1].weight))          # (b)
    s2 = ModelDescriptor.signature(m)
    assert s2 != s1 and ModelDescriptor.signature(m) == s2
    m.load_state_dict(m.state_dict())                                                              # (c)
    s3 = ModelDescriptor.signature(m)
    assert s3 != s2
    m.invalidate_graphs()
    assert ModelDescriptor.signature(m) != s3


def test_partition_properties_hypothesis():
    """esme.shard.partition_sequences on arbitrary length lists and world sizes: a complete, disjoint, deterministic plan with each rank's indices
    ascending; the greedy longest-first rule keeps every load within one longest sequence of the mean (and of every other load); local batches
    rebuilt from the plan carry exactly the owners' tokens."""
    from hypothesis import given, settings, strategies as st
    from esme import shard

    @settings(max_examples=150, deadline=None)
    @given(st.lists(st.integers(min_value=1, max_value=3502), min_size=0, max_size=120), st.integers(min_value=1, max_value=9))
    def check(lens, world):
        plan = shard.partition_sequences(lens, world)
        assert plan == shard.partition_sequences(list(lens), world) and len(plan) == world
        assert sorted(i for p in plan for i in p) == list(range(len(lens))) and all(p == sorted(p) for p in plan)
        if lens:
            loads = [sum(lens[i] for i in p) for p in plan]
            assert max(loads) - min(loads) <= max(lens) and max(loads) <= sum(lens) / world + max(lens)
            tokens = torch.arange(sum(lens), dtype=torch.int64)
            cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
            seen = []
            for p in plan:
                t, c, ml = shard.local_batch(tokens, cu, p)
                assert t.numel() == sum(lens[i] for i in p) and c[0] == 0 and int(c[-1]) == t.numel() and ml == (max(lens[i] for i in p) if p else 0)
                seen.append(t)
            assert torch.equal(torch.sort(torch.cat(seen)).values, tokens)
    check()


# ------------------------------------------------------------------ alignment of every 8- / 16-byte access is checked on the host

_P = 1 << 20          # a 16-byte aligned fake device address: validation happens before anything is dereferenced or launched


def _alignment_table():
    """(entry point, valid arguments, {argument index: a value that breaks the alignment include/esme_hip.h states}).  The valid call passes
    validation (it would launch); each variant must be refused on the host with ESME_ERR_ARG / ESME_ERR_UNSUPPORTED.
    Not listed, because their kernels touch the operand one 2- or 4-byte element at a time: esme_hip_quantize_4bit (w), the cls / w_k operands of
    esme_hip_attn_pool_fold, the output of esme_hip_attn_pool, esme_hip_softmax_rows*, esme_hip_seq_positions / esme_hip_seq_order."""
    P = _P
    cb = (ctypes.c_float * 16)()
    return [
        ('esme_hip_layernorm', [P, 64, P, P, P, 64, 4, 64, 1e-5], {0: P + 2, 1: 68, 4: P + 2, 5: 68}),
        ('esme_hip_layernorm_f32', [P, 64, P, P, P, 64, 4, 64, 1e-5], {0: P + 4, 1: 66, 4: P + 2, 5: 68}),
        ('esme_hip_layernorm_split', [P, 64, 0, 0, P, P, P, 128, 64, P, 64, 4, 64, 1e-5], {0: P + 4, 1: 66, 6: P + 2, 7: 132, 8: 68, 9: P + 4, 10: 66}),
        ('esme_hip_layernorm_split_checked', [P, 128, 1, 64, P, P, P, 128, 64, P, 64, 4, 64, 1e-5, None], {0: P + 2, 1: 132, 3: 68, 6: P + 2}),
        ('esme_hip_rotary_varlen', [P, P, 128, P, P, P, 4, 2, 64, 8], {0: P + 2, 1: P + 2, 2: 132}),
        ('esme_hip_rotary_varlen_f16', [P, P, 128, P, P, P, 4, 2, 64, 8], {0: P + 2, 1: P + 2, 2: 132}),
        ('esme_hip_rotary_split', [P, 512, 256, P, P, P, 4, 2, 64, 8], {0: P + 2, 1: 516, 2: 260}),
        ('esme_hip_rotary_split_f16', [P, 512, 256, P, P, P, 4, 2, 64, 8], {0: P + 2, 1: 516, 2: 260}),
        ('esme_hip_qk_norm_rotary', [P, P, 128, P, P, None, None, 1e-5, P, P, P, 4, 2, 64, 8], {0: P + 2, 1: P + 2, 2: 132}),
        ('esme_hip_qk_norm_rotary_scaled', [P, P, 128, P, P, None, None, 1e-5, P, P, P, 4, 2, 64, 8, 0.18], {0: P + 2, 2: 132}),
        ('esme_hip_qk_norm_rotary_f16', [P, P, 128, P, P, None, None, 1e-5, P, P, P, 4, 2, 64, 8], {0: P + 2, 2: 132}),
        ('esme_hip_qk_norm_rotary_f16_guarded', [P, P, 128, P, P, None, None, 1e-5, P, P, P, 4, 2, 64, 8, None], {0: P + 2, 2: 132}),
        ('esme_hip_qk_norm_rotary_f16_scaled', [P, P, 128, P, P, None, None, 1e-5, P, P, P, 4, 2, 64, 8, 0.18, None], {0: P + 2, 2: 132}),
        ('esme_hip_attn_varlen_fwd', [P, P, P, 384, P, 128, P, 1, 8, 2, 64, 8, 0.125], {0: P + 2, 1: P + 8, 2: P + 2, 3: 388, 4: P + 2, 5: 130}),
        ('esme_hip_attn_varlen_fwd_exact', [P, P, P, 384, P, 128, P, 1, 8, 2, 64, 8, 0.125], {0: P + 2, 3: 388, 4: P + 2, 5: 130}),
        ('esme_hip_attn_varlen_fwd_split', [P, P, P, 768, 384, P, 256, 128, P, 1, 8, 2, 64, 8, 0.125, None], {0: P + 2, 3: 772, 4: 388, 5: P + 2, 6: 258, 7: 130}),          # (o: 8-byte stores, ld_o % 4)
        ('esme_hip_attn_varlen_fwd_qkpair_f16', [P, P, P, 640, 384, P, 128, P, 1, 8, 2, 64, 8, 0.125, None], {0: P + 2, 3: 644, 4: 388, 5: P + 2, 6: 130}),
        ('esme_hip_residual_f32', [P, 64, P, 64, 0.5, 0, P, 64, P, 4, 64], {0: P + 4, 1: 66, 2: P + 2, 3: 68, 6: P + 2, 7: 68}),
        ('esme_hip_stream_operand', [P, 64, P, 128, 64, 1, P, 4, 64], {0: P + 4, 1: 66, 2: P + 2, 3: 132, 4: 68}),
        ('esme_hip_stream_operand_scaled', [P, 64, P, 192, 128, 1, P, None, 0, 0, P, 4, 64], {0: P + 4, 2: P + 2, 3: 196, 4: 132, 6: P + 4}),
        ('esme_hip_pair_to_f32', [P, 128, 64, 1, P, 64, 4, 64], {0: P + 2, 1: 132, 2: 68, 4: P + 4, 5: 66}),
        ('esme_hip_row_sums', [P, 64, 4, 64, P], {0: P + 2, 1: 68}),
        ('esme_hip_gather_rows', [P, 8, P, P, 4, 64], {0: P + 2, 3: P + 2}),
        ('esme_hip_scatter_rows', [P, P, P, 8, 4, 64], {0: P + 2, 2: P + 2}),
        ('esme_hip_segment_mean', [P, 64, P, 2, 64, P, 64, 0], {0: P + 2, 1: 68, 5: P + 2, 6: 68}),
        ('esme_hip_attn_pool_fold', [P, 64, P, 64, 64, 4, 2, P], {7: P + 4}),                    # (cls / w_k: element-wise 2-byte loads)
        ('esme_hip_attn_pool', [P, 64, P, 2, 8, 64, 4, 2, P, P, 1 << 20, P, 128, 0], {0: P + 2, 1: 68, 8: P + 4, 9: P + 4}),      # (out: element-wise stores)
        ('esme_hip_relu_linear', [P, 64, P, 64, P, P, 8, 4, 8, 64, 0], {0: P + 2, 1: 68, 2: P + 2, 3: 68}),
        ('esme_hip_lora_down', [P, 128, P, 8, 4, 64, 64, P, 128], {0: P + 2, 1: 132, 2: P + 2, 7: P + 2, 8: 132}),
        ('esme_hip_gemm_bf16', [P, 64, P, P, None, 0, P, 64, 8, 64, 64, 0, 1.0], {0: P + 2, 1: 68, 2: P + 2, 3: P + 2}),
        ('esme_hip_gemm_qkv_rotary', [P, 64, P, None, P, 192, 8, 192, 64, P, P, P, 64, 8, 128], {0: P + 2, 1: 68, 4: P + 2, 5: 196, 9: P + 2}),
        ('esme_hip_dequantize_4bit', [P, P, 4, 64, cb, None, P, 64], {6: P + 2, 7: 68}),
        ('esme_hip_quantize_8bit', [P, 64, 4, 64, P, P], {0: P + 2, 1: 68}),
        ('esme_hip_dequantize_8bit', [P, P, 4, 64, None, P, 64], {5: P + 2, 6: 68}),
        ('esme_hip_embed', [P, P, P, 4, 64, 33, -1, -1], {1: P + 2, 2: P + 2}),
        ('esme_hip_embed_positions', [P, P, P, P, 2, P, 4, 64, 33, 70, -1], {1: P + 2, 2: P + 2, 5: P + 2}),
        ('esme_hip_embed_positions_f32', [P, P, P, P, 2, P, 4, 64, 33, 70, -1], {1: P + 2, 2: P + 2, 5: P + 4}),
    ]


@pytest.mark.parametrize('name,args,bad', _alignment_table(), ids=[t[0] for t in _alignment_table()])
def test_misaligned_pointer_or_stride_is_refused_before_any_launch(name, args, bad):
    """For every entry point whose kernel uses 8- or 16-byte accesses: a pointer or a leading dimension that breaks the alignment the header
    states returns ESME_ERR_ARG or ESME_ERR_UNSUPPORTED from the host-side checks -- never ESME_OK, and never ESME_ERR_LAUNCH (which would
    mean the call got as far as the launch)."""
    from esme import _hip
    fn = getattr(_hip.load(), name)
    missed = []
    for i, v in bad.items():
        a = list(args)
        a[i] = v
        code = fn(*a, None)
        if code not in (-1, -2):
            missed.append(f'argument {i} = {v:#x}: code {code} ({_hip.load().esme_hip_last_error()})')
    assert not missed, f'{name}: not refused on the host: ' + '; '.join(missed)


# ------------------------------------------------------------------ the row kernels keep a row in registers: widths above 5 120 are refused

_E_WIDE = 5128        # the first multiple of 8 past the widest instantiation (10 chunks of 512 elements)


def _too_wide_table():
    """(entry point, message prefix, arguments that pass every other check with E = _E_WIDE)"""
    P, E = _P, _E_WIDE
    return [
        ('esme_hip_layernorm', b'layernorm', [P, E, P, P, P, E, 4, E, 1e-5]),
        ('esme_hip_residual_f32', b'residual_f32', [P, E, P, E, 0.5, 0, P, E, P, 4, E]),
        ('esme_hip_stream_operand_guarded', b'stream_operand', [P, E, P, E, 0, 0, None, None, 0, 0, P, None, 4, E]),
        ('esme_hip_layernorm_f32', b'layernorm_f32', [P, E, P, P, P, E, 4, E, 1e-5]),
        ('esme_hip_layernorm_split_checked', b'layernorm_split', [P, 2 * E, 1, E, P, P, P, 2 * E, E, P, E, 4, E, 1e-5, None]),
        ('esme_hip_row_sums', b'row_sums', [P, E, 4, E, P]),
    ]


@pytest.mark.parametrize('name,prefix,args', _too_wide_table(), ids=[t[0] for t in _too_wide_table()])
def test_rows_wider_than_5120_are_unsupported_before_any_launch(name, prefix, args):
    """Every entry point that picks its kernel by the row width E refuses E > 5 120 on the host with ESME_ERR_UNSUPPORTED and its own
    '<entry>: E > 5120 unsupported' text (every other argument of these calls is valid, and nothing is launched)."""
    from esme import _hip
    lib = _hip.load()
    assert getattr(lib, name)(*args, None) == -2
    assert lib.esme_hip_last_error() == prefix + b': E > 5120 unsupported'
