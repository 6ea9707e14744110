"""precision 'half', the rules esme.halfmode states once (no device): the staleness rule as the device-side snapshot and the host-side verdict
apply it, the "checks deferred" flag, and the state object a model owns (read-only `_half_guard`, deepcopy, nn.Module.half)."""
import copy
import warnings

import pytest
import torch
from torch import nn

from esme import halfmode
from esme.attention import HalfGuard, HalfPlan
from esme.esm import ESM2

E, L, H = 128, 2, 2
SELECTED = 3


def small_model():
    """ESM2 2 x 128 x 2 with random parameters (LayerNorm gains around 1: the guard sites carry their rho) and a hand-made calibrated plan:
    channel 3 in the extension tile, q / k pairs in layer 1 only (`qk_pair=True` is what makes the per-layer flags count)."""
    torch.manual_seed(0)
    model = ESM2(num_layers=L, embed_dim=E, attention_heads=H)
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(1 + 0.2 * torch.randn(p.shape) if 'norm' in name and name.endswith('weight') else 0.05 * torch.randn(p.shape))
    plan = HalfPlan(torch.tensor([SELECTED], dtype=torch.int32), qk_pair=True, info={'calibrated': True}, qk_layers=[False, True], site_ref=None)
    return model.set_precision('half', robust=plan), plan


@pytest.fixture(scope='module')
def guarded():
    model, plan = small_model()
    model.half_mode.guard = HalfGuard(L, E, H, 'cpu')
    return model, plan, halfmode.guard_scales(model, 'cpu')


def fill(guard, scales, x, sumsq):
    """The guard's bit patterns for stream maxima `x` (2 L + 1, E) in the model's own units and squared q / k row norms `sumsq` (L,)."""
    guard.col.copy_((x * scales).view(torch.int32))
    guard.qk.copy_(sumsq.float()[:, None, None].expand(L, 2, H).contiguous().view(torch.int32))


# head dim 64: score bound = sqrt(q_sumsq * k_sumsq) / 8, so a squared norm of 8 is a bound of 1 and 320 one of 40 (HALF_SCORE_BOUND = 32)
CASES = {
    'benign': (None, [8.0, 8.0], [], []),
    'unselected channel at 10x': ((2, 7, 10.0), [8.0, 8.0], [7], []),
    'selected channel at 50x': ((1, SELECTED, 50.0), [8.0, 8.0], [], []),
    'layer 0 above the score bound': (None, [320.0, 8.0], [], [0]),
    'layer 1 (paired) above the score bound': (None, [8.0, 320.0], [], []),
    'layer 0 without q / k maxima': (None, [0.0, 8.0], [], []),
}


@pytest.mark.parametrize('case', list(CASES))
def test_snapshot_and_verdict_agree(guarded, case, monkeypatch):
    """The device-side snapshot flags a batch exactly when the host-side verdict on that snapshot finds the plan stale, both name the planted
    channels / layers and nothing else, and the snapshot clears the guard."""
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: False)      # (host tensors: no stream; the query itself needs a device)
    model, plan, scales = guarded
    spike, sumsq, channels, layers = CASES[case]
    x = torch.ones(2 * L + 1, E)
    if spike is not None:
        x[spike[0], spike[1]] = spike[2]
    guard = model.half_mode.guard
    fill(guard, scales, x, torch.tensor(sumsq))
    snap = halfmode.guard_snapshot(model)
    assert snap.shape == (1 + E + 2 * L,) and snap[1 + E + L:].tolist() == [float(s > 0) for s in sumsq]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        verdict = halfmode.plan_verdict(model, snap, update=False)
    assert (float(snap[0]) != 0.0) == (verdict is not None) == bool(channels or layers)
    if verdict is not None:
        assert [c for c, _ in verdict['channels']] == channels and [i for i, _ in verdict['layers']] == layers
    assert len([w for w in caught if issubclass(w.category, RuntimeWarning)]) == (verdict is not None)
    assert not bool(guard.col.any()) and not bool(guard.qk.any())
    assert model.half_plan() is plan                                  # (a read-only verdict)


def test_deferred_checks_restore_the_flag_on_every_way_out():
    st = halfmode.HalfState()
    assert st.deferred is False
    with st.deferring():
        assert st.deferred
        with st.deferring():
            assert st.deferred
        assert st.deferred                                            # the inner block restores what IT found
        with st.deferring(False):
            assert st.deferred
    assert st.deferred is False
    with pytest.raises(KeyError):
        with st.deferring():
            with st.deferring():
                raise KeyError('inside')
    assert st.deferred is False
    with st.deferring(False):                                         # (StreamedInference outside precision 'half')
        assert st.deferred is False
    assert st.deferred is False


def test_state_object_delegates_and_copies():
    assert ESM2(num_layers=1, embed_dim=64, attention_heads=1)._half_guard is None
    model, plan = small_model()
    with pytest.raises(AttributeError):
        model._half_guard = None                                      # read-only
    assert not any(isinstance(m, halfmode.HalfState) for m in model.modules()) and 'half_mode' not in dict(model.named_children())
    twin = copy.deepcopy(model)
    assert twin.half_mode is not model.half_mode and twin.half_plan() is not plan and twin.half_plan().ext_key == plan.ext_key
    ratio = torch.ones(E)
    ratio[9] = 20.0
    vec = torch.cat((torch.ones(1), ratio, torch.zeros(L), torch.ones(L)))
    with pytest.warns(RuntimeWarning, match='plan is stale'):
        verdict = halfmode.plan_verdict(twin, vec, update=True)
    assert verdict['updated'] and twin.half_plan().ext_key == (SELECTED, 9)
    assert model.half_plan() is plan and plan.ext_key == (SELECTED,)
    assert model.half.__func__ is nn.Module.half and model.half() is model and model.embed_tokens.weight.dtype == torch.float16
