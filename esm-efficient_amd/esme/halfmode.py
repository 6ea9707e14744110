"""Precision 'half', host side: deciding the plan by a calibration forward (esme.attention.HalfPlan), judging it against the device
maxima (esme.attention.HalfGuard), the sticky range flag, and the checks predict_* / graphed() / esme.pipeline.StreamedInference run around a forward.  One model's state
is one HalfState (`model.half_mode`); the functions take the model explicitly and read the tunables (ESM2.HALF_*, half_*) from it when they use them."""
from __future__ import annotations

import contextlib
import warnings

import torch

from esme.attention import HalfGuard, HalfPlan, _q_scale, has_fixed_reference_form, has_pair_form


class HalfState:
    """Everything precision 'half' keeps per model besides weights: a plain object (no nn.Module, no reference to the model), `model.half_mode`."""

    def __init__(self):
        self.plan = None            # HalfPlan the mode runs with (None: decided on first use -- `half_plan`)
        self.guard = None           # HalfGuard of the forwards since the last check (None before the first 'half' forward / with half_guard off)
        self.ovf = None             # int32 device flag the LayerNorm-folded GEMMs / the final LayerNorm set when a row's statistics are not finite (sticky)
        self.calib = None           # the caller's own calibration batch (tokens int64, cu_lens int32) on the host: set_precision(..., calib=)
        self.probe = None           # a list while the calibration forward runs: collects a torch-side bound of |score| per layer
        self.masks = None           # (plan, selected-channel mask, pair flags) of `plan_masks`, built once per plan and device
        self.deferred = False       # True while a caller reads flag and guard WITH its results (`deferring`): predict_* then check nothing inline

    def overflow_flag(self, device):
        """The sticky range flag on `device` (created on first use)."""
        if self.ovf is None or self.ovf.device != torch.device(device):
            self.ovf = torch.zeros(1, dtype=torch.int32, device=device)
        return self.ovf

    @contextlib.contextmanager
    def deferring(self, on: bool = True):
        """The inline checks of predict_* switched off inside the block (with `on`); the flag is what it was before on every way out."""
        before = self.deferred
        self.deferred = before or bool(on)
        try:
            yield self
        finally:
            self.deferred = before

    def tensors(self) -> list:
        """The device tensors a captured graph must keep alive: the plan's channel list, the guard's maxima, the range flag."""
        keep = [None if self.plan is None else self.plan.ext_sel] + ([] if self.guard is None else [self.guard.col, self.guard.qk]) + [self.ovf]
        return [t for t in keep if t is not None]

    def for_forward(self, model, device):
        """(plan, range flag, guard) of one forward on `device`.  The guard is created with the first 'half' forward (None when half_guard is off), its q norms
        in the unit the forwards of the plan record them in (HalfGuard.q_scaled: the LN-folded projection of an ESM-2 block records q after the plan's q scale);
        the calibration forward fills the guard it installed itself."""
        plan, g = half_plan(model, device), self.guard
        if self.probe is None and not (model.half_guard and len(model.layers)):
            g = None
        elif self.probe is None:
            att = model.layers[0].self_attn
            if g is None or g.col.device != torch.device(device) or g.col.shape != (2 * len(model.layers) + 1, model.phys_dim):
                g = self.guard = HalfGuard(len(model.layers), model.phys_dim, att.num_heads, device)
            if not torch.cuda.is_current_stream_capturing():      # (a capture follows warm-up forwards of the same plan)
                g.rescale_q(plan.qp and not att.pre_layernorm, _q_scale(att.head_dim))
        return plan, self.overflow_flag(device), g


def configure(model, robust=None, calib=None) -> bool:
    """The `robust` / `calib` arguments of ESM2.set_precision; True when the plan was replaced or dropped."""
    st, changed = model.half_mode, False
    if isinstance(robust, HalfPlan):
        st.plan, changed = robust, True
    elif robust is not None:
        assert robust in ('auto', True, False), robust
        if robust != model.half_robust:                       # (only a CHANGE drops the plan: set_precision('half') on a calibrated model keeps it)
            st.plan, changed = None, True
        model.half_robust = robust
    if calib is not None:
        tokens, rest = calib
        cu = rest[0] if isinstance(rest, (tuple, list)) else rest
        st.calib = (tokens.detach().reshape(-1).cpu().to(torch.int64), cu.detach().reshape(-1).cpu().to(torch.int32))
        st.plan, changed = None, True
    return changed


def half_plan(model, device=None):
    st = model.half_mode
    if st.plan is None:
        if model.half_robust is False or not len(model.layers):
            st.plan = HalfPlan(info={'calibrated': False})
        else:
            st.plan = calibrate(model, device if device is not None else model.embed_tokens.weight.device)
    return st.plan


def calibration_batch(model):
    """The built-in calibration input: 8 sequences / 1 024 tokens from numpy PCG64 (the same on every machine) -- residues 4..23 with, for
    HALF_CALIB_VOCAB = 'all', EVERY other id of the alphabet (<unk>, X B U Z O . -, <null_1> / |, <mask>; not <pad>, which never occurs in a
    packed input) sprinkled over 8 interior positions each, <cls> / <eos> at the ends; then the caller's own batch if one was given
    (set_precision(..., calib=)).  Returns (tokens int64, cu_lens int32, max_len) on the host."""
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(20250929))
    al = model.alphabet
    lengths = [192, 160, 160, 128, 128, 96, 96, 64]
    toks = [np.concatenate(([al.cls_idx], rng.integers(4, 24, size=n - 2), [al.eos_idx])) for n in lengths]
    tokens = np.concatenate(toks).astype(np.int64)
    if model.HALF_CALIB_VOCAB == 'all':
        starts = np.concatenate(([0], np.cumsum(lengths)))
        interior = np.ones(tokens.size, dtype=bool)
        interior[starts[:-1]] = False
        interior[starts[1:] - 1] = False
        others = [i for i in range(len(al.alphabet)) if not (4 <= i < 24) and i not in (al.cls_idx, al.eos_idx, al.padding_idx)]
        spots = rng.choice(np.nonzero(interior)[0], size=8 * len(others), replace=False)
        tokens[spots] = np.repeat(np.asarray(others, dtype=np.int64), 8)
    lengths = list(lengths)
    if model.half_mode.calib is not None:
        ut, ucu = model.half_mode.calib
        tokens = np.concatenate((tokens, ut.numpy()))
        lengths += [int(b - a) for a, b in zip(ucu[:-1].tolist(), ucu[1:].tolist())]
    cu = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    return torch.from_numpy(tokens), torch.from_numpy(cu), int(max(lengths))


def guard_scales(model, device):
    """(2 L + 1, phys_dim) float32: the per-column scaling the STORED pair stream carries at each guard site (HalfGuard.col rows): rho of layer 0's
    attention LayerNorm at the start, rho of the FFN LayerNorm after layer i's attention branch, rho of layer i + 1's attention LayerNorm after
    its FFN branch, 1 after the last layer."""
    L = len(model.layers)                   # (stream_scale() is cached per layer on the parameters' versions; this runs at synchronisation points only)
    rows = [model.layers[0].self_attn.stream_scale()[0]]
    for i, layer in enumerate(model.layers):
        rows.append(layer.stream_scale()[0])
        rows.append(model.layers[i + 1].self_attn.stream_scale()[0] if i + 1 < L else torch.ones(model.phys_dim, dtype=torch.float32, device=device))
    return torch.stack([r.to(device) for r in rows])


def guard_measure(model, guard, device, site_ref=None):
    """(channel ratio (E,), score bound per layer (L,), covered (L,) bool, site medians (2 L + 1,)) from a HalfGuard's device maxima -- device
    tensors, no sync.  ratio[c] = max over the sites of  max_t |x[t, c]| / median_c' max_t |x[t, c']|  (0 where a site saw nothing).  `site_ref`:
    the calibration's medians, a floor for the reference (a batch of a few rows has widely scattered per-channel maxima: 1 row of N(0, 1) values
    reaches 6.4 x its median); the medians returned are this guard's own, before that floor."""
    E = model.embed_dim
    x = guard.col.view(torch.float32)[:, :E] / guard_scales(model, device)[:, :E]
    site_med = med = x.median(dim=1).values
    if site_ref is not None:
        med = torch.where(med > 0, torch.maximum(med, site_ref.to(device)), med)
    ratio = torch.where(med[:, None] > 0, x / med[:, None].clamp_min(1e-30), torch.zeros_like(x)).amax(dim=0)
    qk = guard.qk.view(torch.float32)
    att = model.layers[0].self_attn
    # the unit the q norms were RECORDED in (HalfGuard.q_scaled), not the current plan's: a plan change between the forwards and this reading
    # would otherwise mis-scale the bound by softmax_scale * log2(e)
    bound = (qk[:, 0] * qk[:, 1]).sqrt().amax(dim=1) * ((1.0 / 1.4426950408889634) if guard.q_scaled else att.head_dim ** -0.5)
    return ratio, bound, qk.amax(dim=(1, 2)) > 0, site_med


def _largest64(idx, score):
    """The (at most 64) channels of `idx` with the largest `score`, ascending: what fits the extension tile."""
    if idx.numel() > 64:
        idx = idx[torch.argsort(score[idx], descending=True)[:64]]
    return torch.sort(idx).values


def calibrate(model, device):
    """One forward of the plain 'half' form over the calibration batch (calibration_batch: the whole vocabulary, + the caller's own data if
    given), measured by the SAME device maxima the run-time guard keeps (HalfGuard: largest |value| of every stream channel after every
    branch of every layer and at the start relative to the median channel's; squared q / k row norms per head) plus, for blocks
    whose projection does not carry the q / k guard (ESM-C, head dim 128, no rotary), a torch-side bound of |score| per layer."""
    st = model.half_mode
    tokens, cu, max_len = calibration_batch(model)
    tokens, cu = tokens.to(device), cu.to(device)
    att = model.layers[0].self_attn
    L = len(model.layers)
    guard = HalfGuard(L, model.phys_dim, att.num_heads, device)
    saved = (model.precision, st.guard)
    st.plan = HalfPlan(info={'calibrating': True})                      # the plain form, and no recursion
    probe = []
    st.probe, st.guard, model.precision = probe, guard, 'half'
    try:
        with torch.no_grad():
            model._forward_representation(tokens, (cu, max_len), False, None, [L - 1])      # (`layers=`: the module-by-module path, which feeds the probe)
    except BaseException:
        st.plan = None                                                  # (no half-built plan survives a failed calibration)
        raise
    finally:
        st.probe = None
        model.precision, st.guard = saved
    ratio, g_bound, covered, site_med = guard_measure(model, guard, device)
    bounds = [float(b) for b in torch.stack(probe).tolist()] if probe else []        # one per layer, in layer order (torch-side, every layout)
    if len(bounds) == L:                                                              # the kernels' own figure where they keep one: the larger counts
        bounds = [max(b, float(g)) if c else b for b, g, c in zip(bounds, g_bound.tolist(), covered.tolist())]
    bound = max(bounds) if bounds else 0.0
    mass = torch.nonzero(ratio > model.HALF_CHANNEL_RATIO).flatten()
    n_mass = int(mass.numel())
    sel = _largest64(mass, ratio).to(torch.int32).contiguous() if n_mass else None
    pair_ok = has_pair_form(att)
    qk_pair = pair_ok and (bound >= model.HALF_SCORE_BOUND or model.half_robust is True)
    if bound >= model.HALF_SCORE_BOUND and not pair_ok:
        warnings.warn(f"precision='half': attention scores of this model can reach |s| ~ {bound:.0f}, where fp16 q / k cost more than 1e-3, and its block "
                      "(q/k LayerNorm, head dim 128 or a width that is not a multiple of 128) has no q/k-pair form; use precision 'exact' if 1e-3 must hold")
    # the pair form is paid per layer: only where that layer's own bound asks for it (robust=True: everywhere)
    flags = None if (model.half_robust is True or len(bounds) != L) else [b >= model.HALF_SCORE_BOUND for b in bounds]
    others = ratio.clone()
    if sel is not None:
        others[sel.long()] = 0
    info = {'calibrated': True, 'calibration_tokens': int(tokens.numel()), 'vocabulary': model.HALF_CALIB_VOCAB + (' + user batch' if st.calib is not None else ''),
            'max_channel_ratio': float(ratio.max()), 'max_unselected_channel_ratio': float(others.max()), 'score_bound': bound,
            'massive_channels': n_mass, 'qk_pair_supported': bool(pair_ok), 'qk_pair_layers': (L if flags is None else sum(flags)) if qk_pair else 0,
            'score_guard_layers': int(covered.sum()), 'score_bounds': [round(b, 2) for b in bounds]}
    # the fixed-reference form of the fp16 attention kernel (round 6): where the kernels have it and every layer that would use it stays below HALF_QP_BOUND
    plain = [b for i, b in enumerate(bounds) if not (qk_pair and (flags is None or flags[i]))]
    qp = bool(model.half_qp and has_fixed_reference_form(att) and len(bounds) == L and plain and max(plain) < model.HALF_QP_BOUND)
    info['fixed_reference_attention'] = qp
    return HalfPlan(sel, qk_pair, info, qk_layers=flags, site_ref=site_med.clone(), qp=qp)


def plan_masks(model, plan, dev=None):
    """(selected-channel mask (E,) bool, per-layer pair flags (L,) bool) of `plan` on `dev`, built once per plan (None: on the host, not kept)."""
    c = model.half_mode.masks
    if dev is None or c is None or c[0] is not plan or c[1].device != torch.device(dev):
        sel_mask = torch.zeros(model.embed_dim, dtype=torch.bool, device=dev)
        if plan.ext_sel is not None:
            sel_mask[plan.ext_sel.long() if dev is not None else torch.tensor(plan.ext_key, dtype=torch.long)] = True
        c = (plan, sel_mask, torch.tensor([plan.pairs_at(i) for i in range(len(model.layers))], dtype=torch.bool, device=dev))
        if dev is not None:
            model.half_mode.masks = c
    return c[1], c[2]


def stale(ratio, bound, covered, sel_mask, flags, thresholds):
    """THE staleness rule, on tensors of any device: (bad_c (E,), bad_l (L,)) -- the channels outside the extension tile (`sel_mask`) whose
    ratio exceeds thresholds[0] (HALF_CHANNEL_RATIO), the covered layers without q / k pairs (`flags`) whose score bound reaches thresholds[1]
    (HALF_SCORE_BOUND).  The plan is stale when either has a member."""
    return (ratio > thresholds[0]) & ~sel_mask, (bound >= thresholds[1]) & ~flags & covered


def guard_snapshot(model):
    """Device-side half of check_plan (no synchronisation): float32 vector [stale, ratio (E), score bound (L), covered (L)] of everything the
    guard saw since it was last cleared, judged against the CURRENT plan; the maxima are cleared.  None when there is nothing to check.
    esme.pipeline.StreamedInference downloads it with each result."""
    g = model.half_mode.guard
    if g is None or model.precision != 'half' or torch.cuda.is_current_stream_capturing():
        return None
    plan = half_plan(model)
    if not plan.info.get('calibrated', False):
        g.clear()
        return None                                           # (robust=False: the caller asked for the plain form; nothing to hold it to)
    dev = g.col.device
    ratio, bound, covered, _ = guard_measure(model, g, dev, plan.site_ref)
    bad_c, bad_l = stale(ratio, bound, covered, *plan_masks(model, plan, dev), (model.HALF_CHANNEL_RATIO, model.HALF_SCORE_BOUND))
    flag = (bad_c.any() | bad_l.any()).to(torch.float32).reshape(1)
    g.clear()
    return torch.cat((flag, ratio, bound, covered.to(torch.float32)))


def plan_verdict(model, vec, update: bool = True, where: str = ''):
    """Host-side half of check_plan: `vec` = a guard_snapshot() on the host.  None when the plan held; else the verdict dict (and, with
    `update`, the widened plan installed).  What no plan can cover (more than 64 massive channels; large scores in a block without a q/k-pair
    form) leaves the plan, its descriptors and graphs as they are: with `update` it is recorded in plan.info['uncovered'] and warned about once
    per plan; without, nothing is written (and the warning repeats until an updating check has recorded it)."""
    if vec is None or float(vec[0]) == 0.0:
        return None
    st = model.half_mode
    E, L = model.embed_dim, len(model.layers)
    ratio, bound, covered = vec[1:1 + E], vec[1 + E:1 + E + L], vec[1 + E + L:1 + E + 2 * L] > 0
    plan = half_plan(model)
    sel_mask, flags = plan_masks(model, plan)
    bad_c, bad_l = stale(ratio, bound, covered, sel_mask, flags, (model.HALF_CHANNEL_RATIO, model.HALF_SCORE_BOUND))
    if not bool(bad_c.any() | bad_l.any()):
        return None                                           # (judged against a plan that has been widened since the snapshot was taken)
    chans = [(int(c), round(float(ratio[c]), 2)) for c in torch.nonzero(bad_c).flatten().tolist()]
    layers = [(int(i), round(float(bound[i]), 1)) for i in torch.nonzero(bad_l).flatten().tolist()]
    pair_ok = has_pair_form(model.layers[0].self_attn)
    verdict = {'channels': chans, 'layers': layers, 'updated': False}
    msg = (f"precision='half': the plan is stale for this data{where} -- {len(chans)} stream channel(s) outside the extension tile reach "
           f"{max([r for _, r in chans], default=0):.1f}x the median channel (threshold {model.HALF_CHANNEL_RATIO}), "
           f"{len(layers)} layer(s) without q/k pairs reach a score bound of {max([b for _, b in layers], default=0):.0f} (threshold {model.HALF_SCORE_BOUND}); "
           "results computed since the last check may miss the mode's 1e-3.")
    # the widest plan that could cover this: the current selection stays, offenders join (largest first, up to 64); offending layers get pairs where the block has them
    merged = torch.where(sel_mask, torch.full_like(ratio, float('inf')), ratio)
    cand = _largest64(torch.nonzero(sel_mask | bad_c).flatten(), merged)
    new_flags = [bool(f) or (pair_ok and bool(b)) for f, b in zip(flags.tolist(), bad_l.tolist())]
    new_mask = torch.zeros(E, dtype=torch.bool)
    new_mask[cand] = True
    left = ([c for c, _ in chans if not bool(new_mask[c])], [i for i, _ in layers if not new_flags[i]])
    if left[0] or left[1]:
        verdict['uncovered'] = True
    widens = tuple(cand.tolist()) != tuple(plan.ext_key or ()) or new_flags != flags.tolist()
    if not widens:
        # nothing a plan can do about these offenders: the plan stays (no re-run, no new descriptor or graph); say so once per plan
        seen = plan.info.get('uncovered', {'channels': [], 'layers': []})
        new = [c for c in left[0] if c not in seen['channels']], [i for i in left[1] if i not in seen['layers']]
        if update:                                            # (a read-only check does not touch the plan: it warns until an updating one records)
            plan.info['uncovered'] = {'channels': sorted(seen['channels'] + new[0]), 'layers': sorted(seen['layers'] + new[1])}
        if not (new[0] or new[1]):
            verdict['message'] = msg + " (The plan cannot cover this: warned about once for this plan.)"
            return verdict
        msg += (" The plan cannot cover this (more than 64 massive channels, or large scores in a block without a q/k-pair form) and stays as it is; "
                "use precision 'exact' if 1e-3 must hold.  (Said once per plan.)")
    elif update:
        dev = model.embed_tokens.weight.device
        sel = cand.to(torch.int32).contiguous().to(dev) if cand.numel() else None
        info = dict(plan.info)
        info['updates'] = info.get('updates', 0) + 1
        info['massive_channels'] = int(cand.numel())
        info['qk_pair_layers'] = sum(new_flags) if pair_ok else 0
        info['uncovered'] = {'channels': sorted(left[0]), 'layers': sorted(left[1])}      # (already said below: not repeated for this plan)
        st.plan = HalfPlan(sel, pair_ok and any(new_flags), info, qk_layers=new_flags if pair_ok else None, site_ref=plan.site_ref, qp=plan.qp)
        model._drop_derived()
        verdict['updated'] = True
        msg += " The plan was widened (" + st.plan.describe() + "): re-run the batch."
        if verdict.get('uncovered'):
            msg += (" It cannot cover everything (more than 64 massive channels, or large scores in a block without a q/k-pair form): "
                    "use precision 'exact' if 1e-3 must hold.")
    verdict['message'] = msg
    warnings.warn(msg, RuntimeWarning, stacklevel=3)                 # (the caller of ESM2.check_plan / of StreamedInference._hand_out)
    return verdict


def check_overflow(model):
    f = model.half_mode.ovf
    if f is None or torch.cuda.is_current_stream_capturing():
        return model
    if int(f.item()) != 0:
        f.zero_()
        raise OverflowError("precision='half': an activation left IEEE fp16's range (|x| >= 65 504) during a forward since the last check (this call's, "
                            "or an earlier unchecked model(...) call's: the flag is sticky); the result holds inf / NaN.  Use precision 'exact' "
                            "(bf16 pairs, fp32's range) for this checkpoint / input.")
    return model


def checked_run(model, run, tokens=None, recheck: bool = True):
    """Run `run()` (a forward ending in a softmax, or its graph replay) and, in precision 'half' with half_check = 'sync' and the checks not deferred,
    look at the token ids, the range flag and the plan guard (one synchronisation; the result is about to be read anyway).  A stale plan is widened and
    the batch re-run ONCE with it, so the value returned rests on a plan that covers this very batch; an overflow raises.  `recheck`: look at flag and
    guard once more after that re-run (predict_* do; graphed() leaves its second replay's maxima to the next check, as it always has)."""
    y = run()
    if model.precision != 'half' or model.half_check != 'sync' or model.half_mode.deferred:
        return y
    if tokens is not None:
        model.check_tokens(tokens)
    if torch.cuda.is_current_stream_capturing():
        return y
    model.check_overflow()
    v = model.check_plan(update=True)
    if v is not None and v['updated']:                        # (a verdict no plan can cover changes nothing: no re-run)
        y = run()
        if recheck:
            model.check_overflow()
            model.check_plan(update=False)                    # (whatever is left cannot be covered: warned about, not looped on)
    return y
