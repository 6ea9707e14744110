"""precision 'half', host side of the plan's life cycle (no device): esme.halfmode.plan_verdict on hand-made guard vectors and HalfPlans, the plan kept or
dropped by set_precision / invalidate_graphs, and the unit of the guard's q norms (HalfGuard.q_scaled).

A verdict that no plan can cover (more than 64 massive channels; large scores in a block without a q/k-pair form: every ESM-C model) must leave
the plan, its descriptors and graphs alone and warn once per plan -- re-installing an equivalent plan made every predict_* call run two forwards,
rebuild the C descriptor and recapture its graph.
"""
import warnings

import pytest
import torch

from esme import halfmode
from esme.attention import HalfGuard, HalfPlan
from esme.esm import ESM2, ESMC


def vec_of(model, ratio=None, bound=None, covered=None):
    """A guard_snapshot() as it arrives on the host: [stale, ratio (E), score bound (L), covered (L)]."""
    E, L = model.embed_dim, len(model.layers)
    ratio = torch.ones(E) if ratio is None else ratio
    bound = torch.zeros(L) if bound is None else bound
    covered = torch.ones(L) if covered is None else covered
    stale = float(bool((ratio > model.HALF_CHANNEL_RATIO).any() or (bound >= model.HALF_SCORE_BOUND).any()))
    return torch.cat((torch.tensor([stale]), ratio, bound, covered.float()))


def calibrated(sel=None, **kw):
    return HalfPlan(None if sel is None else torch.tensor(sel, dtype=torch.int32), info={'calibrated': True}, **kw)


def sentinel(model):
    """Stand-ins for a C-entry descriptor and a graph cache: what a plan change must drop and a no-op verdict must keep."""
    desc = object()
    model.__dict__['_cdesc16'] = desc
    return desc


def verdicts(model, vec, n, update=True):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        out = [halfmode.plan_verdict(model, vec.clone(), update=update) for _ in range(n)]
    return out, [w for w in caught if issubclass(w.category, RuntimeWarning)]


def test_more_than_64_massive_channels_leave_the_plan_alone_and_warn_once():
    model = ESM2(num_layers=2, embed_dim=256, attention_heads=4)
    full = list(range(0, 128, 2))                                      # 64 channels: the extension tile is full
    plan = calibrated(full)
    model.set_precision('half', robust=plan)
    desc = sentinel(model)
    ratio = torch.ones(256)
    ratio[full] = 50.0
    ratio[[1, 3, 201]] = 9.0                                           # three more massive channels, weaker than every selected one
    out, warned = verdicts(model, vec_of(model, ratio), 3)
    assert all(v is not None and v['updated'] is False and v.get('uncovered') for v in out), out
    assert {c for c, _ in out[0]['channels']} == {1, 3, 201}
    assert len(warned) == 1 and 'cannot cover' in str(warned[0].message)
    assert model.half_plan() is plan and model.__dict__.get('_cdesc16') is desc
    assert plan.info['uncovered'] == {'channels': [1, 3, 201], 'layers': []}
    # a NEW uncoverable offender is news: one more warning, still no new plan
    ratio[77] = 8.0
    out, warned = verdicts(model, vec_of(model, ratio), 2)
    assert len(warned) == 1 and model.half_plan() is plan and model.__dict__.get('_cdesc16') is desc
    # the same holds without `update` (check_plan(update=False) after a re-run)
    out, warned = verdicts(model, vec_of(model, ratio), 2, update=False)
    assert not warned and all(v['uncovered'] and not v['updated'] for v in out)


@pytest.mark.parametrize('kind', ['esmc', 'esm2_d128'])
def test_large_scores_without_a_pair_form_leave_the_plan_alone_and_warn_once(kind):
    """ESM-C (q/k LayerNorm) and head dim 128: no q/k-pair form exists, so a layer at HALF_SCORE_BOUND cannot be covered."""
    model = ESMC(num_layers=3, embed_dim=192, attention_heads=3) if kind == 'esmc' else ESM2(num_layers=3, embed_dim=256, attention_heads=2)
    plan = calibrated()
    model.set_precision('half', robust=plan)
    desc = sentinel(model)
    bound = torch.tensor([3.0, 40.0, 33.0])
    out, warned = verdicts(model, vec_of(model, bound=bound), 2, update=False)          # a read-only check warns and writes nothing
    assert len(warned) == 2 and all(v['uncovered'] and not v['updated'] for v in out) and 'uncovered' not in plan.info
    out, warned = verdicts(model, vec_of(model, bound=bound), 3)
    assert all(v['updated'] is False and v['uncovered'] for v in out), out
    assert [i for i, _ in out[0]['layers']] == [1, 2]
    assert len(warned) == 1
    assert model.half_plan() is plan and model.__dict__.get('_cdesc16') is desc and not plan.qk_pair


def test_a_verdict_that_widens_installs_one_new_plan():
    """Coverable offenders: a new plan with the channels joined / the layers paired, descriptors dropped, one warning; the same data is then covered."""
    model = ESM2(num_layers=3, embed_dim=256, attention_heads=4)             # head dim 64, width 256: the pair form exists
    plan = calibrated([5, 9], qp=True)
    plan.site_ref = torch.ones(7)
    model.set_precision('half', robust=plan)
    desc = sentinel(model)
    ratio = torch.ones(256)
    ratio[[5, 9]] = 30.0
    ratio[[40, 41]] = 12.0
    bound = torch.tensor([2.0, 50.0, 1.0])
    vec = vec_of(model, ratio, bound)
    out, warned = verdicts(model, vec, 1)
    v = out[0]
    assert v['updated'] and not v.get('uncovered') and len(warned) == 1
    new = model.half_plan()
    assert new is not plan and new.ext_key == (5, 9, 40, 41) and new.qk_layers == (False, True, False) and new.qp and new.site_ref is plan.site_ref
    assert '_cdesc16' not in model.__dict__ and new.info['updates'] == 1
    out, warned = verdicts(model, vec, 2)
    assert out == [None, None] and not warned and model.half_plan() is new


def test_a_widening_that_still_leaves_offenders_warns_once_for_both_plans():
    """Channels beyond the 64 of the tile: the first verdict widens (the strongest join) and says what is left; the re-run's check under the new
    plan does not repeat it, and nothing is re-installed."""
    model = ESM2(num_layers=2, embed_dim=256, attention_heads=4)
    plan = calibrated(list(range(60)))
    model.set_precision('half', robust=plan)
    ratio = torch.ones(256)
    ratio[:60] = 40.0
    ratio[100:110] = torch.arange(10, 20, dtype=torch.float32)
    vec = vec_of(model, ratio)
    out, warned = verdicts(model, vec, 1)
    assert out[0]['updated'] and out[0]['uncovered'] and len(warned) == 1
    new = model.half_plan()
    assert new.ext_key == tuple(range(60)) + (106, 107, 108, 109)
    assert new.info['uncovered'] == {'channels': list(range(100, 106)), 'layers': []}
    desc = sentinel(model)
    out, warned = verdicts(model, vec, 2)
    assert not warned and all(v['uncovered'] and not v['updated'] for v in out)
    assert model.half_plan() is new and model.__dict__.get('_cdesc16') is desc


def test_invalidate_graphs_recalibrates_and_set_precision_keeps_the_plan():
    """invalidate_graphs() (the documented step after editing weights in place) drops the plan: the next 'half' forward recalibrates on the edited
    weights.  set_precision and a widening verdict only drop what is derived from the plan they install."""
    model = ESM2(num_layers=2, embed_dim=128, attention_heads=2)
    plan = calibrated([3])
    model.set_precision('half', robust=plan)
    assert model.half_plan() is plan
    model.set_precision('fast')
    model.set_precision('half')
    assert model.half_plan() is plan                                         # a mode switch keeps it
    sentinel(model)
    model._drop_derived()
    assert model.half_plan() is plan and '_cdesc16' not in model.__dict__
    sentinel(model)
    model.invalidate_graphs()
    assert model.half_mode.plan is None and '_cdesc16' not in model.__dict__
    model.set_precision('half', robust=plan)
    model.load_state_dict(model.state_dict())
    assert model.half_mode.plan is None


def test_guard_q_norms_convert_between_units():
    """HalfGuard.q_scaled: the q norms recorded after the projection's q scale (an ESM-2 plan with the fixed-reference form) and before it (every other
    plan) convert into each other; k norms and the column maxima do not move; zeros stay zeros."""
    from esme.attention import _q_scale
    g = HalfGuard(3, 64, 4, 'cpu')
    q2 = torch.tensor([[1.5, 2.0, 0.0, 7.25]] * 3)
    g.qk.view(torch.float32)[:, 0] = q2
    g.qk.view(torch.float32)[:, 1] = 3.0
    g.col.view(torch.float32)[:] = 0.5
    col, k = g.col.clone(), g.qk[:, 1].clone()
    qs = _q_scale(64)
    g.rescale_q(False, qs)                                                    # same unit: nothing happens
    assert torch.equal(g.qk.view(torch.float32)[:, 0], q2)
    g.rescale_q(True, qs)
    assert g.q_scaled and torch.allclose(g.qk.view(torch.float32)[:, 0].double(), q2.double() * qs * qs, rtol=1e-6, atol=0)
    g.rescale_q(True, qs)
    g.rescale_q(False, qs)
    assert not g.q_scaled and torch.allclose(g.qk.view(torch.float32)[:, 0], q2, rtol=1e-6, atol=0)
    assert torch.equal(g.qk[:, 1], k) and torch.equal(g.col, col) and float(g.qk.view(torch.float32)[0, 0, 2]) == 0.0


def _changed(get, edit, model):
    before = get().clone()
    edit()
    model.invalidate_graphs()
    return not torch.equal(before, get())


def test_invalidate_graphs_rebuilds_every_derived_weight_copy_after_p_data_writes():
    """A `p.data` write moves no version counter: invalidate_graphs() must still make EVERY derived weight copy follow it -- the LN-folded fp16 QKV /
    up-projection weights with the extension K-tile of a plan with massive channels, ESM-C's packed SwiGLU weight, the padded copies of a layout
    whose heads are padded (ESM2-35M-like), the fp16 out-projection -- and leave them alone without an edit."""
    torch.manual_seed(0)
    sel = torch.tensor([3, 7, 64], dtype=torch.int32)
    m = ESM2(num_layers=1, embed_dim=128, attention_heads=2)
    for p in m.parameters():
        p.data.normal_()
    att, layer = m.layers[0].self_attn, m.layers[0]
    w0 = att._weights_qkv(True, True, sel)[0].clone()
    m.invalidate_graphs()
    assert torch.equal(att._weights_qkv(True, True, sel)[0], w0)                                     # nothing edited: the same values
    assert _changed(lambda: att._weights_qkv(True, True, sel)[0], lambda: att.q.weight.data.mul_(6.0), m)
    assert _changed(lambda: layer._weights_up(True, True, sel)[0], lambda: layer.final[1].weight.data.mul_(3.0), m)
    assert _changed(lambda: att._weights_out(True)[0], lambda: att.out.weight.data.mul_(3.0), m)
    c = ESMC(num_layers=1, embed_dim=192, attention_heads=3)
    for p in c.parameters():
        p.data.normal_()
    sw = c.layers[0].final[1]
    assert _changed(lambda: c.layers[0]._weights_up(True, True)[0], lambda: sw.activation.weight.data.mul_(3.0), c)
    assert _changed(lambda: c.layers[0]._weights_up(True, True, sel)[0], lambda: sw.fc.weight.data.mul_(0.5), c)
    pm = ESM2(num_layers=1, embed_dim=96, attention_heads=4)                                         # head dim 24 -> 32, width 96 -> 128
    for p in pm.parameters():
        p.data.normal_()
    patt = pm.layers[0].self_attn
    assert pm.padded
    assert _changed(lambda: patt._weights_qkv(True, True)[0], lambda: patt.k.weight.data.mul_(6.0), pm)
    assert _changed(lambda: patt._weights_out(True)[0], lambda: patt.out.weight.data.mul_(2.0), pm)
    assert _changed(lambda: pm.layers[0]._weights_up(False)[0], lambda: pm.layers[0].final[1].weight.data.mul_(2.0), pm)
