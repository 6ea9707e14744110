"""CPU tests of the attention-pooling heads (esme/pooling.py, esme/head.py, csrc/pool.hip): the folded algebra against the
reference's definition in float64, state-dict layouts, argument refusals of the C entry points (library loaded, no GPU), and the
per-element bound of tests/attn_pool_bounds.py against CPU emulations of the kernel, correct and with defects."""
import ctypes
import math

import pytest
import torch

import attn_pool_bounds as apb
from error_bounds import assert_bounded


def _operands(lengths, E, H, C, seed, x_dtype=torch.bfloat16, score_gain=1.0):
    g = torch.Generator().manual_seed(seed)
    T = sum(lengths)
    x = torch.randn(T, E, generator=g).to(x_dtype)
    cls = (torch.randn(C, E, generator=g) * score_gain).to(torch.bfloat16)
    wk = (torch.randn(E, E, generator=g) / math.sqrt(E)).to(torch.bfloat16)
    bk = (torch.randn(E, generator=g) * 0.1).to(torch.bfloat16)
    cu = torch.tensor([0] + list(torch.tensor(lengths).cumsum(0)), dtype=torch.int32)
    return x, cu, cls, wk, bk


def test_reference_restatement_equals_folded_form_in_float64():
    """The literal reference data flow (k with bias, softmax(q k / sqrt d) v) equals the folded form u . x / sqrt d, k bias 1e3 included."""
    x, cu, cls, wk, _ = _operands([5, 70, 1, 130], 64, 4, 3, seed=1)
    bk = torch.full((64,), 1e3)
    ref, p = apb.reference_pool(x, cu, cls, wk, bk, 4)
    ref0, _ = apb.reference_pool(x, cu, cls, wk, torch.zeros(64), 4)
    assert torch.allclose(ref, ref0, rtol=0, atol=1e-9)
    # softmax of the folded scores reproduces p
    z = apb.folded_scores(x, cls, wk, 4)
    cu_l = cu.long()
    for b in range(4):
        zs = z[cu_l[b]:cu_l[b + 1]]
        assert torch.allclose(torch.softmax(zs, dim=0), p[cu_l[b]:cu_l[b + 1]], rtol=1e-12, atol=1e-15)


REF_KEYS = {
    'AttentionPool': ['k.weight', 'k.bias'],
    'LearnedAttentionPool': ['cls', 'k.weight', 'k.bias'],
    'LearnedAggregation': ['attn.cls', 'attn.k.weight', 'attn.k.bias', 'linear.weight', 'linear.bias', 'final.weight', 'final.bias'],
    'BinaryLearnedAggregation': ['attn.cls', 'attn.k.weight', 'attn.k.bias', 'linear.weight', 'linear.bias', 'final.weight',
                                 'final.bias'],
    'ClsHead': ['head.0.weight', 'head.0.bias', 'head.2.weight', 'head.2.bias'],
}


def test_state_dict_keys_match_the_reference():
    from esme.head import ClsHead
    from esme.pooling import AttentionPool, BinaryLearnedAggregation, LearnedAggregation, LearnedAttentionPool
    mods = {'AttentionPool': AttentionPool(4, 256), 'LearnedAttentionPool': LearnedAttentionPool(4, 4, 512),
            'LearnedAggregation': LearnedAggregation(4, 4, 512), 'BinaryLearnedAggregation': BinaryLearnedAggregation(4, 512),
            'ClsHead': ClsHead(512, 1024)}
    for name, m in mods.items():
        assert set(m.state_dict()) == set(REF_KEYS[name]), name
        assert all(not p.requires_grad for p in m.parameters()), name
    la = mods['LearnedAttentionPool']
    assert la.cls.shape == (4, 512) and bool((la.cls == 1).all())
    assert mods['ClsHead'].head[2].weight.shape == (1024, 4096)
    # fp32 tensors (a head trained with dtype=torch.float32) cast into the bf16 parameters
    sd = {k: v.float() * 0.5 for k, v in mods['BinaryLearnedAggregation'].state_dict().items()}
    m = BinaryLearnedAggregation(4, 512)
    m.load_state_dict(sd)
    assert m.linear.weight.dtype == torch.bfloat16 and torch.equal(m.linear.weight, sd['linear.weight'].to(torch.bfloat16))


def test_refusals_in_python():
    from esme.pooling import AttentionPool, BinaryLearnedAggregation, LearnedAggregation
    with pytest.raises(NotImplementedError):
        AttentionPool(4, 256, dropout_p=0.1)
    with pytest.raises(NotImplementedError):
        BinaryLearnedAggregation(4, 256, dropout_p=0.1)
    with pytest.raises(ValueError):
        LearnedAggregation(1, 3, 256)                  # 256 % 3 != 0
    with pytest.raises(ValueError):
        AttentionPool(2, 36)                           # E % 8 != 0
    pool = AttentionPool(4, 256)
    with pytest.raises(TypeError):
        pool(torch.ones(1, 256), torch.ones(3, 256, dtype=torch.float16), (torch.tensor([0, 3]), 3))


def test_c_entry_points_refuse_bad_arguments():
    from esme import _hip
    lib = _hip.load()
    # workspace query: geometry checks
    assert lib.esme_hip_attn_pool_workspace_bytes(2, 100, 256, 4, 1) == (2 + 1 + 1) * (2 * 4 + 256) * 4
    assert lib.esme_hip_attn_pool_workspace_bytes(2, 100, 256, 3, 1) == -1            # E % heads
    assert lib.esme_hip_attn_pool_workspace_bytes(2, 100, 36, 4, 1) == -1             # E % 8
    assert lib.esme_hip_attn_pool_workspace_bytes(-1, 100, 256, 4, 1) == -1           # negative B
    assert lib.esme_hip_attn_pool_workspace_bytes(2, 100, 1280, 20, 26) == -2         # J = 520 > 512
    assert lib.esme_hip_attn_pool_workspace_bytes(2, 100, 1280, 32, 16) == (2 + 1 + 1) * (2 * 512 + 16 * 1280) * 4
    # fold
    assert lib.esme_hip_attn_pool_fold(None, 256, 16, 256, 256, 4, 1, 16, None) == -1
    assert lib.esme_hip_attn_pool_fold(16, 256, 16, 256, 256, 4, 1, 8, None) == -1           # misaligned U
    assert lib.esme_hip_attn_pool_fold(16, 128, 16, 256, 256, 4, 1, 16, None) == -1         # ldc < E
    assert lib.esme_hip_attn_pool_fold(16, 512, 16, 512, 512, 4, 129, 16, None) == -2        # J > 512
    # pool: (x, ldx, cu, B, T, E, H, C, U, ws, ws_bytes, out, ldo, f32, stream)
    ws = 1 << 20
    assert lib.esme_hip_attn_pool(16, 256, 16, 0, 0, 256, 4, 1, 16, 16, ws, 16, 256, 0, None) == 0     # B = 0: no-op
    assert lib.esme_hip_attn_pool(None, 256, 16, 2, 10, 256, 4, 1, 16, 16, ws, 16, 256, 0, None) == -1
    assert lib.esme_hip_attn_pool(16, 256, None, 2, 10, 256, 4, 1, 16, 16, ws, 16, 256, 0, None) == -1
    assert lib.esme_hip_attn_pool(16, 256, 16, 2, 10, 256, 4, 1, 16, None, ws, 16, 256, 0, None) == -1
    assert lib.esme_hip_attn_pool(8, 256, 16, 2, 10, 256, 4, 1, 16, 16, ws, 16, 256, 0, None) == -1      # misaligned x
    assert lib.esme_hip_attn_pool(16, 260, 16, 2, 10, 256, 4, 1, 16, 16, ws, 16, 256, 0, None) == -1     # ldx % 8 (bf16)
    assert lib.esme_hip_attn_pool(16, 128, 16, 2, 10, 256, 4, 1, 16, 16, ws, 16, 256, 0, None) == -1     # ldx < E
    assert lib.esme_hip_attn_pool(16, 256, 16, 2, 10, 256, 4, 2, 16, 16, ws, 16, 256, 0, None) == -1     # ldo < n_cls E
    assert lib.esme_hip_attn_pool(16, 256, 16, 2, 10, 256, 4, 1, 16, 16, 64, 16, 256, 0, None) == -1     # workspace too small
    assert lib.esme_hip_attn_pool(16, 1280, 16, 2, 10, 1280, 20, 26, 16, 16, ws, 16, 26 * 1280, 0, None) == -2   # J > 512
    assert lib.esme_hip_attn_pool(16, 250, 16, 2, 10, 250, 5, 1, 16, 16, ws, 16, 250, 0, None) == -1     # E % 8
    # relu_linear: (h, ldh, w, ldw, b, y, ldy, M, N, K, f32, stream)
    assert lib.esme_hip_relu_linear(16, 64, 16, 64, None, 16, 1, 0, 1, 64, 0, None) == 0                # M = 0: no-op
    assert lib.esme_hip_relu_linear(16, 64, 16, 64, None, 16, 65, 4, 65, 64, 0, None) == -2             # N > 64
    assert lib.esme_hip_relu_linear(None, 64, 16, 64, None, 16, 1, 4, 1, 64, 0, None) == -1
    assert lib.esme_hip_relu_linear(16, 60, 16, 60, None, 16, 1, 4, 1, 60, 0, None) == -1               # K % 8
    assert lib.esme_hip_relu_linear(8, 64, 16, 64, None, 16, 1, 4, 1, 64, 0, None) == -1                # misaligned h
    assert lib.esme_hip_relu_linear(16, 64, 16, 64, None, 16, 1, 4, 0, 64, 0, None) == -1               # N = 0


# ------------------------------------------------------------------ the bound against emulations

CASES = [  # (lengths, E, H, C, x dtype, score gain)
    ([1, 0, 200, 64, 65, 17], 64, 4, 2, torch.bfloat16, 1.0),
    ([130, 3, 129], 96, 4, 1, torch.float32, 1.0),
    ([150, 40, 0, 1], 48, 2, 3, torch.bfloat16, 6.0),         # scores of tens to hundreds
]


@pytest.mark.parametrize('case', range(len(CASES)))
def test_bound_accepts_the_emulated_kernel(case):
    lengths, E, H, C, xdt, gain = CASES[case]
    x, cu, cls, wk, bk = _operands(lengths, E, H, C, seed=10 + case, x_dtype=xdt, score_gain=gain)
    ref, bound = apb.check_pool_inputs(x, cu, cls, wk, bk, H, 'fp32' if xdt == torch.float32 else 'bf16')
    got = apb.emulate_pool(x, cu, cls, wk, H, xdt)
    worst = assert_bounded(got, ref, bound, f'emulated attn_pool case {case}')
    print(f'case {case}: worst err/bound {worst:.3f}')


DEFECTS = ['u_bf16', 'chunk_drop', 'chunk_repeat', 'no_rescale', 'scale_d', 'k_as_v', 'neighbour_head', 'round_twice']


@pytest.mark.parametrize('defect', DEFECTS)
def test_bound_rejects_emulated_defects(defect):
    # two long sequences (several chunks, different chunk maxima) and a short one; bf16 output for the double rounding
    lengths, E, H, C = [300, 7, 190], 64, 4, 2
    x, cu, cls, wk, bk = _operands(lengths, E, H, C, seed=3, score_gain=3.0)
    if defect == 'no_rescale':
        x[0:64] *= 3                                   # the first chunk's maxima differ from the others'
    xdt = torch.float32 if defect == 'u_bf16' else torch.bfloat16
    x = x.to(xdt)
    ref, bound = apb.check_pool_inputs(x, cu, cls, wk, bk, H, 'fp32' if xdt == torch.float32 else 'bf16')
    assert_bounded(apb.emulate_pool(x, cu, cls, wk, H, xdt), ref, bound, 'correct emulation')
    with pytest.raises(AssertionError, match='out of bound'):
        assert_bounded(apb.emulate_pool(x, cu, cls, wk, H, xdt, defect=defect), ref, bound, f'defect {defect}')
