"""precision 'half': the plan and its run-time guard across CHANGES of state -- a plan switched between filling the guard and reading it, weights
edited in place, a stale plan no plan can cover, a hipGraph captured after unchecked forwards or on a batch that widens the plan -- and the
fp16 attention kernel's dispatch for q_prescaled outside the ping-pong kernel.  The steady state (one plan, eager forwards, a plan that can
always be widened) is tests/test_half_guard_gpu.py.

  * HalfGuard.q_scaled: the LN-folded projection records q's norms AFTER its q_scale (HalfPlan.qp on an ESM-2 block), ESM-C's q / k pass before
    it; the guard carries the unit it was filled in and converts when a plan of the other unit runs, so a plan change between the forwards and
    check_plan() reads the same bound (it was mis-scaled by softmax_scale * log2(e) ~ 5.5 at d = 64, and under-read going qp on -> off);
  * invalidate_graphs() recalibrates: a plan decided on the old weights is not held against the edited ones;
  * a verdict no plan can cover changes nothing: one forward per predict_* call, one capture per graphed shape, one warning per plan;
  * a graph capture warms up on the caller's batch with the checks deferred, keeps the guard's maxima and checks once after its first replay.
"""
import warnings

import pytest
import torch

from oracle import esm_oracle as O
from esme import _hip
from esme import synthetic as syn
from esme import halfmode
from esme.attention import HalfPlan, _q_scale
from test_attn_qp16_gpu import prescale, reference
from test_half_guard_gpu import sprinkled, token_outlier_model
from test_model_gpu import build

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H16 = torch.float16


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def as_f32(t):
    return t.view(torch.float32)


def args_of(tokens, cu, lengths):
    return tokens.to(DEV), (cu.to(DEV), max(lengths))


def runtime_warnings(caught):
    return [w for w in caught if issubclass(w.category, RuntimeWarning)]


# ---- A: what the projection epilogue's qk_sumsq records with and without q_scale ------------------------------------------------------------

@pytest.mark.parametrize('tile', [1, 2])
@pytest.mark.parametrize('d,H', [(64, 4), (32, 8), (16, 16)])
def test_projection_qk_row_norms_with_the_q_scale(d, H, tile):
    """esme_gemm_fusion_t.qk_sumsq with q_scale on and off (one loud row, one loud head of q): q's recorded norms are those of the STORED fp16 q
    (scaled when q_scale is on: the unit HalfGuard.q_scaled names) to 1e-5 and q_scale^2 times the unscaled ones to fp16's rounding; k's are
    bit-identical either way; the projection's output is bit-identical with and without the guard, and only q moves with q_scale."""
    from esme.attention import _fold_layernorm_pow2
    from esme.rotary import RotaryEmbedding
    E, K, M = H * d, 256, 1500
    g = torch.Generator().manual_seed(7 * d + tile)
    x = torch.randn(M, K, generator=g)
    x[M // 3] *= 9.0
    gamma = (1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16)
    beta = (0.05 * torch.randn(K, generator=g)).to(torch.bfloat16)
    w = (torch.randn(3 * E, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    w[d:2 * d] *= 6.0
    bias = (0.1 * torch.randn(3 * E, generator=g)).to(torch.bfloat16)
    wf, c1, c2, rho, _ = _fold_layernorm_pow2(w, bias, gamma, beta)
    xs = torch.empty(M, 2 * K, dtype=H16, device=DEV)
    sums = torch.empty(1, M, 2, dtype=torch.float32, device=DEV)
    _hip.stream_operand(x.to(DEV), xs, sums, pair=True, scale=rho.to(DEV))
    lengths = [M // 2, M - M // 2]
    pos, _ = _hip.seq_positions(syn.cu_lens_of(lengths).to(DEV), M)
    cos, sin = RotaryEmbedding(dim=d).tables(max(lengths), DEV, H16)
    qs = _q_scale(d)
    outs, guards = {}, {}
    for scale in (0.0, qs):
        for guarded in (False, True):
            qk = torch.zeros(2, H, dtype=torch.int32, device=DEV) if guarded else None
            with _hip.gemm_options(tile=tile):
                outs[scale, guarded] = _hip.gemm_fused(xs[:, :K], wf.to(DEV), None, ln=(sums, K, 1e-5, c1.to(DEV), c2.to(DEV), None),
                                                       rot=(cos, sin, pos, d, 2 * E), q_scale=scale, qk_sumsq=qk)
            guards[scale, guarded] = qk
    for scale in (0.0, qs):
        assert torch.equal(outs[scale, False], outs[scale, True])
    assert torch.equal(outs[0.0, True][:, E:], outs[qs, True][:, E:])              # k and v: the same bits
    assert torch.equal(guards[0.0, True][1], guards[qs, True][1])                  # k's norms: the same bits
    for scale in (0.0, qs):
        q = outs[scale, True][:, :E].double().cpu().reshape(M, H, d)
        want = q.pow(2).sum(dim=-1).amax(dim=0)
        got = as_f32(guards[scale, True])[0].double().cpu()
        assert torch.allclose(got, want, rtol=1e-5, atol=0), (scale, got, want)
    plain, scaled = (as_f32(guards[s, True])[0].double().cpu() for s in (0.0, qs))
    assert torch.allclose(scaled, plain * qs * qs, rtol=2e-3, atol=0)              # (q rounded to fp16 after vs before the scale)
    assert float(plain[1]) > 8 * float(plain[0])


# ---- B: the guard's score bound across a plan change ---------------------------------------------------------------------------------------

def _fed_bounds(model, args):
    """One module-path forward; per layer, float64 (max_t |q_t|, max_t |k_t|) per head of the q / k the layer handed to attention (q divided by the
    q scale where it arrived prescaled); None for layers that never got there (q/k pairs)."""
    seen = {}
    atts = [layer.self_attn for layer in model.layers]
    for i, att in enumerate(atts):
        inner = att._attn

        def spy(q, k, v, *a, _i=i, _inner=inner, _att=att, **kw):
            qd = q.double().reshape(q.shape[0], _att.num_heads, -1)
            if kw.get('q_prescaled'):
                qd = qd / _q_scale(_att.head_dim)
            kd = k.double().reshape(k.shape[0], _att.num_heads, -1)
            qn, kn = qd.norm(dim=-1).amax(dim=0), kd.norm(dim=-1).amax(dim=0)
            seen[_i] = (qn, kn)
            return _inner(q, k, v, *a, **kw)
        att._attn = spy
    model.c_forward = False
    try:
        model(*args)
    finally:
        model.c_forward = True
        for att in atts:
            del att._attn
    return [seen.get(i) for i in range(len(atts))]


def _bound(model, qn, kn):
    """max_h max_t |q_t| max_t |k_t| d^-0.5"""
    return float((qn * kn).amax()) * model.layers[0].self_attn.head_dim ** -0.5


def _flip_qp(model):
    p = model.half_plan()
    model.set_precision('half', robust=HalfPlan(p.ext_sel, p.qk_pair, p.info, qk_layers=p.qk_layers, site_ref=p.site_ref, qp=not p.qp))
    return model.half_plan()


@pytest.mark.parametrize('case', ['esm2_qp', 'esmc', 'esm2_pairs'])
def test_guard_bound_is_the_fed_q_k_bound_across_a_plan_change(case):
    """guard_measure's per-layer score bound equals a float64 recomputation from what each layer fed to attention; a guard filled under qp = True and
    read after the plan switched to qp = False (and the other way round) reports the same bound, and forwards under the new plan merge into it."""
    lengths = [90, 33, 257]
    tokens, cu = syn.random_tokens(lengths, seed=6), syn.cu_lens_of(lengths)
    args = args_of(tokens, cu, lengths)
    if case == 'esmc':
        model = build('esmc', 2, 960, 15, seed=9)
    else:
        model = build('esm2', 3, 640, 10, seed=9)
        if case == 'esm2_pairs':                       # layer 0's scores beyond HALF_SCORE_BOUND: q/k pairs there, the single form elsewhere
            with torch.no_grad():
                model.layers[0].self_attn.q.weight.mul_(12.0)
                model.layers[0].self_attn.k.weight.mul_(12.0)
    model.set_precision('half')
    plan = model.half_plan()
    if case == 'esm2_pairs':
        assert plan.pairs_at(0) and not plan.pairs_at(1), plan.describe()
    else:
        assert plan.qp, plan.describe()
    model(*args)                                       # (creates the model's guard)
    # ESM-C's q / k pass measures the fp32 values before their fp16 rounding (tests/test_half_guard_gpu.py::test_qk_norm_rotary_pass_row_norms):
    # its bound matches the fed values to that rounding only; the projection epilogue measures exactly what it stores
    tol = 2e-4 if case == 'esmc' else 1e-5
    for flip in range(2):
        model.half_mode.guard.clear()
        fed = _fed_bounds(model, args)
        _, bound, covered, _ = halfmode.guard_measure(model, model.half_mode.guard, DEV)
        bound, covered = bound.cpu().tolist(), covered.cpu().tolist()
        checked = [i for i, f in enumerate(fed) if f is not None and covered[i]]
        assert len(checked) == len(model.layers) - (1 if case == 'esm2_pairs' else 0), (fed, covered)
        for i in checked:
            want = _bound(model, *fed[i])
            assert abs(bound[i] - want) <= tol * want, (case, flip, i, bound[i], want)
        _flip_qp(model)                                # (qp on -> off, then off -> on)
        after = halfmode.guard_measure(model, model.half_mode.guard, DEV)[1].cpu().tolist()
        for i in checked:
            assert abs(after[i] - bound[i]) <= 1e-6 * bound[i], (case, flip, i, after[i], bound[i])
        # a forward under the new plan merges into the same maxima: per head, the larger q norm of the two forwards times the larger k norm
        fed2 = _fed_bounds(model, args)
        merged = halfmode.guard_measure(model, model.half_mode.guard, DEV)[1].cpu().tolist()
        for i in checked:
            want = _bound(model, torch.maximum(fed[i][0], fed2[i][0]), torch.maximum(fed[i][1], fed2[i][1]))
            assert abs(merged[i] - want) <= tol * want, (case, flip, i, merged[i], want)
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            assert model.check_plan(update=False) is None


# ---- C: weights edited in place -------------------------------------------------------------------------------------------------------------

# (model, heads, q / k factor): 'esm2' is the issue's recipe (benign weights with the fixed-reference form on, q / k x 6); 'esm2_ext' a plan with
# extension-tile channels (the fp16 QKV / up weights with the tile appended are copies of their own); 'esmc' the packed SwiGLU weight; 'esm2_padded'
# an ESM2-35M-like layout (head dim 24 padded to 32: padded q / k / v / out copies)
C_CASES = {'esm2': 6.0, 'esm2_x2': 2.0, 'esm2_ext': 2.0, 'esmc': 6.0, 'esm2_padded': 2.0}


def _c_model(kind):
    if kind in ('esm2', 'esm2_x2'):
        return build('esm2', 2, 640, 10, seed=3), 10
    if kind == 'esm2_ext':
        return token_outlier_model('esm2', 2, 640, 20, 50.0, [24, 3])[0], 20
    if kind == 'esmc':
        return build('esmc', 2, 960, 15, seed=9), 15
    return build('esm2', 2, 480, 20, seed=3), 20


def _c_edit(model, factor, how):
    """q / k x factor and the FFN's first weight x 1/2, in place -- through `p.data` (no version counter moves) or under no_grad."""
    for layer in model.layers:
        ffn = layer.final[1]
        pairs = [(layer.self_attn.q.weight, factor), (layer.self_attn.k.weight, factor),
                 (ffn.activation.weight if hasattr(ffn, 'activation') else ffn.weight, 0.5)]
        for p, f in pairs:
            if how == 'data':
                p.data.mul_(f)
            else:
                with torch.no_grad():
                    p.mul_(f)


def _c_run(kind, how, args):
    model, H = _c_model(kind)
    model.set_precision('half')
    model(*args)
    before = model.half_plan()
    _c_edit(model, C_CASES[kind], how)
    model.invalidate_graphs()
    y = model(*args)
    return model, H, before, y


@pytest.mark.parametrize('kind', ['esm2', 'esm2_ext', 'esmc', 'esm2_padded'])
@pytest.mark.parametrize('how', ['data', 'no_grad'])
def test_weight_edits_then_invalidate_graphs_recalibrate(how, kind):
    """Calibrated on the unedited weights, q / k and the FFN's first weight scaled in place, invalidate_graphs(): the next 'half' forward runs the plan a
    fresh model calibrates on the edited weights (same plan) and every derived weight copy follows the edit -- logits bit-identical to that model's."""
    lengths = [50, 120, 7]
    tokens, cu = syn.random_tokens(lengths, seed=1), syn.cu_lens_of(lengths)
    args = args_of(tokens, cu, lengths)
    model, H, before, y = _c_run(kind, how, args)
    fresh, _ = _c_model(kind)
    _c_edit(fresh, C_CASES[kind], 'no_grad')
    y_fresh = fresh.set_precision('half')(*args)
    p, q = model.half_plan(), fresh.half_plan()
    assert p is not before
    assert (p.describe(), p.qp, p.info['score_bound'], p.ext_key) == (q.describe(), q.qp, q.info['score_bound'], q.ext_key), (p.describe(), q.describe())
    if kind == 'esm2':
        assert before.qp and not p.qp, (before.describe(), p.describe())          # the plan of the old weights would have kept the form on
    if kind == 'esm2_ext':
        assert before.ext_sel is not None and p.ext_sel is not None, (before.describe(), p.describe())
    assert torch.equal(y, y_fresh)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert model.check_plan(update=False) is None


@pytest.mark.parametrize('kind', [
    pytest.param('esm2', marks=pytest.mark.xfail(strict=True, reason=(
        'q / k x 6 leaves an ill-conditioned model (score bound ~530): a 2^-11 relative perturbation of its weights moves the fp32 logits by ~2e-2 '
        '(~1.5e-3 for the unedited weights), so fp16 operands cannot reach 1e-3 under ANY plan -- a freshly calibrated model measures the same '
        '5e-3 -- and the guard cannot see it (it thresholds channel ratios and score bounds, not conditioning)'))),
    'esm2_x2', 'esm2_ext', 'esmc', 'esm2_padded'])
def test_edited_weights_half_vs_oracle(kind):
    """The recalibrated 'half' forward on the edited weights is within 1e-3 of the fp32 oracle on those weights."""
    lengths = [50, 120, 7]
    tokens, cu = syn.random_tokens(lengths, seed=1), syn.cu_lens_of(lengths)
    model, H, _, y = _c_run(kind, 'data', args_of(tokens, cu, lengths))
    w = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ref = O.forward_logits(w, H, tokens, cu, max(lengths), torch.float32).float()
    err = rel(y.float().cpu(), ref)
    print(f'\n[lifecycle] {kind}: {model.half_plan().describe()}, score bound {model.half_plan().info["score_bound"]:.1f}, half vs fp32 oracle {err:.2e}')
    assert err <= 1e-3, err


# ---- D: a stale plan no plan can cover ----------------------------------------------------------------------------------------------------

def _uncoverable(kind):
    if kind == 'esmc':                                   # q / k LayerNorm gains: scores beyond HALF_SCORE_BOUND in a block without a pair form
        model = build('esmc', 2, 960, 15, seed=4)
        with torch.no_grad():
            for layer in model.layers:
                layer.self_attn.layernorm_q.weight.mul_(5.0)
                layer.self_attn.layernorm_k.weight.mul_(5.0)
        return model
    # more than 64 massive channels: 80 columns at +-50 in every residue's embedding row (the counter-example models of test_half_guard_gpu.py)
    w, _ = syn.token_outlier_state_dict('esm2', 2, 640, 50.0, list(range(4, 24)), seed=2, n_channels=80, gain_scale=1.0)
    model = build('esm2', 2, 640, 10, seed=2)
    model.load_state_dict({k: v.clone() for k, v in w.items()}, strict=False)
    return model.to(DEV)


def _n_channels(model):
    return int(model.half_plan().ext_sel.numel()) if model.half_plan().ext_sel is not None else 0


@pytest.mark.parametrize('kind', ['esmc', 'esm2_80ch'])
def test_uncoverable_verdict_changes_nothing_and_warns_once(kind, monkeypatch):
    """A verdict no plan can cover (ESM-C scores beyond HALF_SCORE_BOUND; 80 massive channels for a 64-wide tile) leaves everything as it is: after the
    first call, one forward per predict_log_prob, the same plan and C descriptor, one capture for three graphed calls (bit-equal to eager),
    check_plan() says updated = False, uncovered = True -- and one RuntimeWarning for the plan."""
    from esme import graph as G
    model = _uncoverable(kind)
    lengths = [60, 130, 21]
    tokens, cu = syn.random_tokens(lengths, seed=2), syn.cu_lens_of(lengths)
    args = args_of(tokens, cu, lengths)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                  # (the calibration's own note on scores it cannot cover)
        model.set_precision('half').half_plan()
    if kind == 'esm2_80ch':
        assert _n_channels(model) == 64 and model.half_plan().info['massive_channels'] > 64, model.half_plan().info
    calls = []
    inner = model._forward_representation
    model._forward_representation = lambda *a, **kw: (calls.append(1), inner(*a, **kw))[1]
    captures = []
    real_capture = G.GraphedForward._capture
    monkeypatch.setattr(G.GraphedForward, '_capture', lambda self: (captures.append(1), real_capture(self))[1])
    plans = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        first = model.predict_log_prob(*args)
        plan, desc = model.half_plan(), model.__dict__.get('_cdesc16')
        plans.append(plan)
        assert desc is not None
        for _ in range(2):
            calls.clear()
            again = model.predict_log_prob(*args)
            assert len(calls) == 1
            assert model.half_plan() is plan and model.__dict__.get('_cdesc16') is desc
            assert torch.equal(again, first)
        graphed = [model.graphed(*args, what='predict_log_prob') for _ in range(3)]
        assert len(captures) == 1 and all(torch.equal(gy, first) for gy in graphed)
        assert model.half_plan() is plan
        model(*args)
        v = model.check_plan()
        assert v is not None and v['updated'] is False and v['uncovered'] is True, v
        assert model.half_plan() is plan and model.__dict__.get('_cdesc16') is desc
    stale = [w for w in runtime_warnings(caught) if 'plan is stale' in str(w.message)]
    assert len(stale) == len(plans) == 1, [str(w.message) for w in stale]


# ---- E: graph warm-up and capture ---------------------------------------------------------------------------------------------------------

def test_graph_capture_keeps_what_unchecked_forwards_saw():
    """An unchecked model(...) on a batch with token-triggered channels the calibration missed, then a graphed capture on a benign batch: the next
    check_plan() still reports the stale plan (the capture used to clear the maxima)."""
    model, _, cols = token_outlier_model('esm2', 4, 640, 20, 50.0, [24, 3], vocab='residues')
    model.set_precision('half')
    assert model.half_plan().ext_sel is None
    lengths = [150, 61, 300]
    bad, cu = sprinkled(lengths, [24, 3], 0.2)
    model(*args_of(bad, cu, lengths))
    good_lengths = [40, 25]
    good = syn.random_tokens(good_lengths, seed=9)
    model.graphed(*args_of(good, syn.cu_lens_of(good_lengths), good_lengths))
    with pytest.warns(RuntimeWarning, match='plan is stale'):
        v = model.check_plan(update=False)
    assert v is not None and set(cols.tolist()) <= {c for c, _ in v['channels']}, v


def test_first_graphed_predict_on_a_triggering_batch(monkeypatch):
    """A first graphed predict_log_prob on a batch that shows the plan stale: it ends with the widened plan, returns what eager predict_log_prob returns
    under that plan (bit for bit; within 1e-3 of the fp32 oracle), and no graph entry is cleared while it is being captured."""
    from esme import graph as G
    model, w, cols = token_outlier_model('esm2', 4, 640, 20, 50.0, [24, 3], vocab='residues')
    model.set_precision('half')
    assert model.half_plan().ext_sel is None
    lengths = [150, 61, 300]
    tokens, cu = sprinkled(lengths, [24, 3], 0.2)
    args = args_of(tokens, cu, lengths)
    capturing, cleared_inside = [], []
    real_capture, real_clear = G.GraphedForward._capture, G.GraphCache.clear

    def capture(self):
        capturing.append(self)
        try:
            return real_capture(self)
        finally:
            capturing.pop()

    def clear(self):
        if capturing:
            cleared_inside.append(len(self.entries))
        return real_clear(self)
    monkeypatch.setattr(G.GraphedForward, '_capture', capture)
    monkeypatch.setattr(G.GraphCache, 'clear', clear)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        y = model.graphed(*args, what='predict_log_prob')
    assert not cleared_inside
    assert len([m for m in runtime_warnings(caught) if 'plan is stale' in str(m.message)]) == 1
    plan = model.half_plan()
    assert plan.ext_sel is not None and set(cols.tolist()) <= set(plan.ext_sel.tolist()), plan.describe()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        eager = model.predict_log_prob(*args)
    assert model.half_plan() is plan and torch.equal(y, eager)
    ref = torch.log_softmax(O.forward_logits(w, 20, tokens, cu, max(lengths), torch.float32).double(), dim=-1).float()
    assert rel(y.float().cpu(), ref) <= 1e-3


def test_graphed_predict_checks_the_token_ids():
    """graphed predict_log_prob validates the caller's token ids after every replay, as the eager call does (the capture's warm-up defers the
    checks).  An id outside the table is read as a zero embedding row by the kernel: nothing out of bounds happens before the check raises."""
    model = build('esm2', 2, 320, 20, seed=4).set_precision('half')
    lengths = [30, 17]
    tokens, cu = syn.random_tokens(lengths, seed=2), syn.cu_lens_of(lengths)
    args = args_of(tokens, cu, lengths)
    model.graphed(*args, what='predict_log_prob')
    bad = tokens.clone()
    bad[5] = 99
    for _ in range(2):                                      # the first replay of the captured shape and a second one
        with pytest.raises(IndexError):
            model.graphed(*args_of(bad, cu, lengths), what='predict_log_prob')


# ---- F: fp16 attention with q_prescaled outside the ping-pong kernel ------------------------------------------------------------------------

@pytest.mark.parametrize('variant', [0, 1, 2, 4, 8])
@pytest.mark.parametrize('d,H', [(64, 6), (32, 10)])
def test_prescaled_f16_attention_every_variant_vs_float64(variant, d, H):
    """Variants 1 and 2 have no prescaled fp16 form: they run the generic kernel with a unit scale.  Every variant: within 6e-4 of float64 on the same
    fp16 inputs; a sequence alone equals the same sequence packed, bit for bit."""
    lengths = [5, 64, 333, 1, 130, 700]
    T, E = sum(lengths), H * d
    g = torch.Generator().manual_seed(3 * d + variant)
    q, k, v = (torch.randn(T, E, generator=g).to(H16) for _ in range(3))
    qs = prescale(q, d)
    cu = syn.cu_lens_of(lengths)
    with _hip.attn_options(variant=variant):
        out = _hip.attn_varlen(qs.to(DEV), k.to(DEV), v.to(DEV), cu.to(DEV), max(lengths), H, q_prescaled=True)
        assert bool(torch.isfinite(out).all())
        assert rel(out.cpu(), reference(qs, k, v, cu, H, d)) <= 6e-4, variant
        cl = cu.tolist()
        for i in (2, 5):
            s0, s1 = cl[i], cl[i + 1]
            alone = _hip.attn_varlen(qs[s0:s1].to(DEV), k[s0:s1].to(DEV), v[s0:s1].to(DEV), syn.cu_lens_of([s1 - s0]).to(DEV), s1 - s0, H,
                                     q_prescaled=True)
            assert torch.equal(alone, out[s0:s1]), (variant, i)


def test_prescaled_f16_attention_beyond_32bit_offsets():
    """THE LARGE-MEMORY TEST of this file (one 4.6 GB allocation): a row stride of 2^21 elements with 1 100 rows, so that (max_len + 64) rows do not fit
    the ping-pong kernel's 32-bit byte offsets -- the generic kernel runs with a unit scale.  Only the 192 live columns (q, k, v of 64 each) are
    written; the result is within 6e-4 of float64."""
    H, d, S, ld = 1, 64, 1100, 1 << 21
    assert (S + 64) * ld * 2 >= 1 << 32
    g = torch.Generator().manual_seed(21)
    q, k, v = (torch.randn(S, H * d, generator=g).to(H16) for _ in range(3))
    qs = prescale(q, d)
    buf = torch.empty(S, ld, dtype=H16, device=DEV)
    try:
        buf[:, 0:64] = qs.to(DEV)
        buf[:, 64:128] = k.to(DEV)
        buf[:, 128:192] = v.to(DEV)
        cu = syn.cu_lens_of([S])
        out = _hip.attn_varlen(buf[:, 0:64], buf[:, 64:128], buf[:, 128:192], cu.to(DEV), S, H, q_prescaled=True)
        assert bool(torch.isfinite(out).all())
        assert rel(out.cpu(), reference(qs, k, v, cu, H, d)) <= 6e-4
    finally:
        del buf
        torch.cuda.empty_cache()
