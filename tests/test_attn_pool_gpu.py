"""GPU tests of the attention-pooling kernels (csrc/pool.hip) and the heads on them (esme/pooling.py, esme/head.py).

Every check is per element, |got - ref64| <= bound with no rms floor: ref64 is the float64 restatement of the reference's data flow
(tests/attn_pool_bounds.py: k projected with its bias, softmax(q k^T / sqrt d) v) on the operands the kernel was handed, and the bound
is the sum of the kernel's rounding steps.  There are no reference goldens for these heads: the reference imports flash_attn."""
import math

import pytest
import torch

import attn_pool_bounds as apb
from error_bounds import U32, assert_bounded, out_round

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _hip():
    from esme import _hip
    _hip.load()
    return _hip


def _operands(lengths, E, H, C, seed, x_dtype=torch.bfloat16, score_gain=1.0, device=DEV):
    g = torch.Generator().manual_seed(seed)
    T = sum(lengths)
    x = torch.randn(T, E, generator=g).to(x_dtype).to(device)
    cls = (torch.randn(C, E, generator=g) * score_gain).to(torch.bfloat16).to(device)
    wk = (torch.randn(E, E, generator=g) / math.sqrt(E)).to(torch.bfloat16).to(device)
    bk = (torch.randn(E, generator=g) * 0.1).to(torch.bfloat16).to(device)
    cu = torch.zeros(len(lengths) + 1, dtype=torch.int32)
    cu[1:] = torch.tensor(lengths).cumsum(0)
    return x, cu.to(device), cls, wk, bk


def _pool(x, cu, cls, wk, H):
    hip = _hip()
    U = hip.attn_pool_fold(cls, wk, H)
    return hip.attn_pool(x, cu, U, H, cls.shape[0])


def _fmt(x):
    return 'fp32' if x.dtype == torch.float32 else 'bf16'


RAGGED = [1, 0, 300, 77, 5, 130, 64, 0, 65]
GEOMS = [(4, 256), (4, 512), (20, 320), (20, 480), (20, 960), (20, 1280), (40, 2560)]


@pytest.mark.parametrize('H,E', GEOMS)
@pytest.mark.parametrize('x_dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('n_cls', [1, 4, 16])
def test_pool_within_bound(H, E, x_dtype, n_cls):
    x, cu, cls, wk, bk = _operands(RAGGED, E, H, n_cls, seed=E + n_cls, x_dtype=x_dtype)
    if n_cls * H > 512:                                                  # (40, 2560) with 16 class tokens: J = 640
        with pytest.raises(RuntimeError, match='code -2'):
            _pool(x, cu, cls, wk, H)
        return
    got = _pool(x, cu, cls, wk, H)
    assert got.dtype == x_dtype and got.shape == (len(RAGGED), n_cls, E)
    ref, bound = apb.check_pool_inputs(x, cu, cls, wk, bk, H, _fmt(x))
    assert_bounded(got, ref, bound, f'attn_pool H={H} E={E} n_cls={n_cls} {x_dtype}')
    assert bool((got[[1, 7]] == 0).all())                                # zero-length sequences pool to zeros


def test_pool_refuses_too_many_queries():
    x, cu, cls, wk, _ = _operands([3, 4], 1280, 20, 26, seed=0)
    with pytest.raises(RuntimeError, match='code -2'):
        _pool(x, cu, cls, wk, 20)


def test_pool_one_long_sequence():
    """One 35 000-row sequence: 547 chunks merged by the combine launch."""
    x, cu, cls, wk, bk = _operands([35000], 1280, 20, 1, seed=5)
    ref, bound = apb.check_pool_inputs(x, cu, cls, wk, bk, 20, 'bf16')
    assert_bounded(_pool(x, cu, cls, wk, 20), ref, bound, 'attn_pool 35 000 rows')


def test_pool_70002_short_sequences():
    g = torch.Generator().manual_seed(11)
    lengths = torch.randint(0, 13, (70002,), generator=g).tolist()
    x, cu, cls, wk, bk = _operands(lengths, 320, 20, 2, seed=12)
    ref, bound = apb.check_pool_inputs(x, cu, cls, wk, bk, 20, 'bf16')
    assert_bounded(_pool(x, cu, cls, wk, 20), ref, bound, 'attn_pool B = 70 002')


def test_pool_scores_in_the_hundreds():
    x, cu, cls, wk, bk = _operands([500, 64, 129, 1], 320, 20, 4, seed=13, x_dtype=torch.float32, score_gain=40.0)
    z = apb.folded_scores(x, cls, wk, 20)
    assert float(z.abs().max()) > 100.0
    ref, bound = apb.check_pool_inputs(x, cu, cls, wk, bk, 20, 'fp32')
    assert_bounded(_pool(x, cu, cls, wk, 20), ref, bound, 'attn_pool large scores')


def test_pool_embed_over_2_31_elements():
    """T * E > 2^31: the last sequences live past element 2^31 of x (64-bit row offsets)."""
    E, H = 1280, 20
    T = (1 << 31) // E + 3000
    lengths = [T - 2700 - 300 - 1, 2700, 300, 1]
    x = torch.empty(T, E, dtype=torch.bfloat16, device=DEV).normal_()
    _, cu, cls, wk, bk = _operands([1], E, H, 1, seed=14)
    cu = torch.tensor([0] + list(torch.tensor(lengths).cumsum(0)), dtype=torch.int32, device=DEV)
    got = _pool(x, cu, cls, wk, H)
    a = int(cu[1])
    tail = x[a:]
    cu_t = (cu[1:] - a).to(torch.int32)
    ref, bound = apb.check_pool_inputs(tail, cu_t, cls, wk, bk, H, 'bf16')
    assert_bounded(got[1:], ref, bound, 'attn_pool past 2^31 elements')
    del x


def test_pool_alone_vs_packed_and_determinism():
    E, H, C = 320, 20, 4
    x, cu, cls, wk, _ = _operands([130, 1, 64, 200, 0, 65], E, H, C, seed=21)
    first = _pool(x, cu, cls, wk, H)
    assert torch.equal(first, _pool(x, cu, cls, wk, H))                  # two runs
    cu_l = cu.tolist()
    for s in (0, 3, 5):
        rows = x[cu_l[s]:cu_l[s + 1]]
        alone = _pool(rows.contiguous(), torch.tensor([0, rows.shape[0]], dtype=torch.int32, device=DEV), cls, wk, H)
        assert torch.equal(alone[0], first[s]), s
        for pad_front in (1, 63, 777):                                   # the same rows behind other sequences
            filler = torch.randn(pad_front, E, device=DEV).to(torch.bfloat16)
            xx = torch.cat([filler, rows, filler[:5]])
            cc = torch.tensor([0, pad_front, pad_front + rows.shape[0], xx.shape[0]], dtype=torch.int32, device=DEV)
            assert torch.equal(_pool(xx, cc, cls, wk, H)[1], first[s]), (s, pad_front)


def test_zero_cls_is_the_mean():
    hip = _hip()
    for dt in (torch.bfloat16, torch.float32):
        x, cu, cls, wk, bk = _operands([1, 90, 300, 64], 480, 20, 3, seed=22, x_dtype=dt)
        cls = torch.zeros_like(cls)
        got = _pool(x, cu, cls, wk, 20)
        mean = hip.segment_mean(x, cu)
        ref, bound = apb.check_pool_inputs(x, cu, cls, wk, bk, 20, _fmt(x))
        lens = (cu[1:] - cu[:-1]).double().view(-1, 1)
        ref_mean = ref[:, 0]
        # segment_mean: fp32 sum of n terms (n U32 relative on sum |x|), a multiply by fp32(1/n), one rounding
        absmean = torch.zeros_like(ref_mean).index_add_(0, torch.repeat_interleave(torch.arange(4, device=DEV), (cu[1:] - cu[:-1]).long()),
                                                        x.double().abs()) / lens
        pre_m = U32 * (lens + 2) * absmean
        bm = pre_m + out_round(ref_mean, pre_m, _fmt(x))
        for c in range(3):
            assert_bounded(got[:, c], mean.double(), bound[:, c] + bm, f'cls = 0 vs segment_mean {dt} c={c}')


def test_k_bias_does_not_change_the_output():
    from esme.pooling import LearnedAttentionPool
    m = LearnedAttentionPool(2, 20, 320).to(DEV)
    x, cu, _, _, _ = _operands([40, 70], 320, 20, 1, seed=23)
    a = m(x, (cu, 70))
    with torch.no_grad():
        m.k.bias.data.normal_(0, 1000.0)
    b = m(x, (cu, 70))
    assert torch.equal(a, b)
    ref, bound = apb.check_pool_inputs(x, cu, m.cls, m.k.weight, m.k.bias, 20, 'bf16')
    assert_bounded(b, ref, bound, 'k bias 1e3')


# ------------------------------------------------------------------ heads

def _randomise(m, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_((torch.randn(p.shape, generator=g) * scale / math.sqrt(max(p.shape[-1], 1))).to(p.dtype))
    return m


def _head_check(mod, embed, cu, H, num_cls, pool_mod):
    """(got, ref64, bound) of final(relu(linear(pool))) on this embed."""
    got = mod(embed, (cu, 0))
    pooled = pool_mod(embed, (cu, 0))
    ref_p, bound_p = apb.check_pool_inputs(embed, cu, pool_mod.cls, pool_mod.k.weight, pool_mod.k.bias, H, _fmt(embed))
    n, c, E = pooled.shape
    y, by = apb.mlp_bound(pooled.reshape(n * c, E), bound_p.reshape(n * c, E) * 0, mod.linear.weight, mod.linear.bias,
                          mod.final.weight, mod.final.bias, _fmt(embed))
    # the pooled values are checked against ref_p above; the head is then checked on those same values
    assert_bounded(pooled, ref_p, bound_p, 'pooled inside the head')
    return got, y.view(n, c, 1).squeeze(1), by.view(n, c, 1).squeeze(1)


@pytest.mark.parametrize('x_dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('E,H', [(512, 4), (480, 20)])
def test_learned_aggregation_heads(x_dtype, E, H):
    from esme.pooling import BinaryLearnedAggregation, LearnedAggregation
    x, cu, _, _, _ = _operands([125, 500, 1, 66], E, H, 1, seed=31, x_dtype=x_dtype)
    la = _randomise(LearnedAggregation(4, H, E), 32).to(DEV)
    got, ref, bound = _head_check(la, x, cu, H, 4, la.attn)
    assert got.shape == (4, 4, 1) and got.dtype == x_dtype
    assert_bounded(got, ref, bound, f'LearnedAggregation {E} {x_dtype}')
    bl = _randomise(BinaryLearnedAggregation(H, E), 33).to(DEV)
    got, ref, bound = _head_check(bl, x, cu, H, 1, bl.attn)
    got = got.squeeze(-1)
    assert got.shape == (4,)
    assert_bounded(got, ref.squeeze(-1), bound.squeeze(-1), f'BinaryLearnedAggregation {E} {x_dtype}')


@pytest.mark.parametrize('x_dtype', [torch.bfloat16, torch.float32])
def test_cls_head(x_dtype):
    from esme.head import ClsHead
    hip = _hip()
    x, cu, _, _, _ = _operands([3, 5, 200], 480, 4, 1, seed=41, x_dtype=x_dtype)
    for num_cls, hidden in ((1, 4096), (100, 512)):
        head = _randomise(ClsHead(480, num_cls=num_cls, hidden_dim=hidden), 42).to(DEV)
        got = head(x, cu)
        pooled = hip.segment_mean(x, cu)
        y, by = apb.mlp_bound(pooled, torch.zeros_like(pooled, dtype=torch.float64), head.head[0].weight, head.head[0].bias,
                              head.head[2].weight, head.head[2].bias, _fmt(x))
        assert got.shape == ((3,) if num_cls == 1 else (3, num_cls)) and got.dtype == x_dtype
        assert_bounded(got.view(3, num_cls), y, by, f'ClsHead num_cls={num_cls} {x_dtype}')


def test_reference_test_shapes():
    """The reference's tests/test_pooling.py and test_head.py shapes as known answers."""
    from esme.head import ClsHead
    from esme.pooling import AttentionPool, BinaryLearnedAggregation, LearnedAggregation, LearnedAttentionPool
    cu = torch.tensor([0, 125, 625], dtype=torch.int32, device=DEV)
    e256 = torch.randn(625, 256, device=DEV).to(torch.bfloat16)
    e512 = torch.randn(625, 512, device=DEV).to(torch.bfloat16)
    cls = torch.randn(1, 256, device=DEV).to(torch.bfloat16)
    assert AttentionPool(4, 256).to(DEV)(cls, e256, (cu, 500)).shape == (2, 1, 256)
    assert LearnedAttentionPool(4, 4, 512).to(DEV)(e512, (cu, 500)).shape == (2, 4, 512)
    assert LearnedAggregation(4, 4, 512).to(DEV)(e512, (cu, 500)).shape == (2, 4, 1)
    assert BinaryLearnedAggregation(4, 512).to(DEV)(e512, (cu.long(), 500)).shape == (2,)
    assert LearnedAggregation(1, 4, 512).to(DEV)(e512, (cu, 500)).shape == (2, 1)
    out = ClsHead(512, 1024).to(DEV)(torch.randn(8, 512, device=DEV).to(torch.bfloat16), torch.tensor([0, 3, 8], device=DEV))
    assert out.shape == (2, 1024)


def test_fp32_state_dict_in_reference_layout_loads_and_runs():
    from esme.pooling import BinaryLearnedAggregation
    E, H = 320, 20
    g = torch.Generator().manual_seed(51)
    sd = {'attn.cls': torch.randn(1, E, generator=g), 'attn.k.weight': torch.randn(E, E, generator=g) / math.sqrt(E),
          'attn.k.bias': torch.randn(E, generator=g), 'linear.weight': torch.randn(E, E, generator=g) / math.sqrt(E),
          'linear.bias': torch.randn(E, generator=g) * 0.1, 'final.weight': torch.randn(1, E, generator=g) / math.sqrt(E),
          'final.bias': torch.randn(1, generator=g)}
    m = BinaryLearnedAggregation(H, E)
    m.load_state_dict(sd)
    m = m.to(DEV)
    x, cu, _, _, _ = _operands([30, 300, 2], E, H, 1, seed=52)
    got, ref, bound = _head_check(m, x, cu, H, 1, m.attn)
    assert_bounded(got.squeeze(-1), ref.squeeze(-1), bound.squeeze(-1), 'fp32 state dict')


@pytest.mark.parametrize('precision', ['fast', 'exact'])
@pytest.mark.parametrize('E,H', [(320, 20), (480, 20)])
def test_gb1_pattern_end_to_end(tmp_path, precision, E, H):
    """workflow/gb1_aav: BinaryLearnedAggregation(H, E * (1 + len(layers))) over forward_representation(..., layers=[...])."""
    from esme import ESM, synthetic as syn
    from esme.pooling import BinaryLearnedAggregation
    L, layers, lengths = 2, [0, 1], [60, 9, 140]
    path = syn.write_checkpoint(str(tmp_path / 'm.safetensors'), 'esm2_gb1', L, E, H, seed=3)
    model = ESM.from_pretrained(path, device=DEV)
    if precision == 'exact':
        model.set_precision('exact')
    tokens, cu = syn.random_tokens(lengths, 4).to(DEV), syn.cu_lens_of(lengths).to(DEV)
    rep = model.forward_representation(tokens, (cu, max(lengths)), layers=layers)
    W = E * (1 + len(layers))
    assert rep.shape == (sum(lengths), W)
    head = _randomise(BinaryLearnedAggregation(H, W), 61).to(DEV)
    got, ref, bound = _head_check(head, rep.contiguous(), cu, H, 1, head.attn)
    assert got.dtype == rep.dtype
    assert_bounded(got.squeeze(-1), ref.squeeze(-1), bound.squeeze(-1), f'gb1 head {precision} E={E}')
