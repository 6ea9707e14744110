"""esme.optim.AdamW in training runs on the device: the tiny ESM-2 (E = 128, H = 4) and ESM-C (E = 128, H = 2, SwiGLU) fixtures with
mark_trainable, LoRA adapters and a BinaryLearnedAggregation head.

What is at stake: the kernel writes parameters through raw pointers, so (1) every derived weight of the package -- keyed on the
parameter's version counter -- must see the update, and (2) at the small learning rates full fine-tuning uses, the update must land, which
it does not on bf16 parameters without fp32 masters.  (2) is measured against three host-side shadows stepped by torch.optim.AdamW on
the model's own gradients: float64 (the truth), float32 and bfloat16.  The printed per-tensor values of a run are kept in
profiles/optim_parity.txt."""
import io
import warnings

import pytest
import torch
import torch.nn.functional as F

import esme
import error_bounds as eb
from golden_util import load_golden
from test_head_train_gpu import make_head
from test_lora_gpu import golden_model, tiny

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KINDS = ('esm2', 'esmc')
_G = {}


def _golden():
    if not _G:
        _G.update(load_golden('g13_lora.npz'))                                # the fixture models' geometry
        _G.update({k: v for k, v in load_golden('g15_full_grad.npz').items() if '/' not in k})      # the masked training batch
    return _G


def _model(tmp_path, kind):
    g = _golden()
    return tiny(tmp_path, kind, *(int(g[f'{kind}_{k}']) for k in ('L', 'E', 'H', 'seed')))


def _batch(kind):
    g = _golden()
    pad_args = (g['cu_lens'].to(DEV), int(g['max_len']))
    labels = ((pad_args[0][1:] - pad_args[0][:-1]).float() / pad_args[1]).to(DEV)
    return dict(tokens_in=g[f'{kind}_tokens_in'].to(DEV), tokens=g[f'{kind}_tokens'].to(DEV), mask=g[f'{kind}_mask'].to(DEV), pad_args=pad_args, labels=labels)


def _head():
    return make_head('BinaryLearnedAggregation', seed=21).to(DEV).requires_grad_(True)


def _head_loss(model, head, b, frozen=False):
    """MSE of the pooling head on per-protein labels (the reference's RegressionTrainer): gradients for backbone and head."""
    if frozen:
        with torch.no_grad():
            rep = model.forward_representation(b['tokens'], b['pad_args'])
    else:
        rep = model.forward_trainable(b['tokens'], b['pad_args'], logits=False)
    return F.mse_loss(head.forward_trainable(rep, b['pad_args']).float(), b['labels'], reduction='sum')


def _lm_loss(model, b, mask=None):
    logits = model.forward_trainable(b['tokens_in'], b['pad_args'])
    return esme.cross_entropy(logits, b['tokens'], b['mask'] if mask is None else mask, alphabet=model.alphabet)


def _backward(loss_fn, modules):
    for m in modules:
        m.zero_grad(set_to_none=True)
    loss = loss_fn()
    loss.backward()
    return loss.detach()


def _trainable(module):
    return [p for p in module.parameters() if p.requires_grad]


def _grads(modules):
    return {f'{i}.{n}': p.grad.clone() for i, m in enumerate(modules) for n, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('kind', KINDS)
def test_updates_reach_every_forward(tmp_path, kind):
    """After the caches of every forward are populated, three steps on the backbone and a head; a fresh model loaded from the trained
    state_dict then computes the same bits everywhere.  A parameter whose version counter the step did not bump would leave a stale
    derived weight (W^T of the dX GEMM, an LN-folded or packed copy) in the trained model and differ here."""
    b = _batch(kind)
    model, head = _model(tmp_path, kind), _head()
    before = model(b['tokens'], b['pad_args']).clone()                       # the inference forward: packed / folded copies
    model.mark_trainable().train()
    opt = esme.optim.AdamW([{'params': _trainable(model)}, {'params': list(head.parameters()), 'lr': 3e-3}], lr=1e-3)
    loss_fn = lambda: _head_loss(model, head, b)
    first = _backward(loss_fn, (model, head))                                # a training step's forward and backward: weight_t
    for _ in range(3):
        opt.step()
        last = _backward(loss_fn, (model, head))
    assert float(last) != float(first)
    want_loss, want_grads = last, _grads((model, head))
    want_logits = model.eval()(b['tokens'], b['pad_args']).clone()
    assert not torch.equal(want_logits, before)
    fresh, fresh_head = _model(tmp_path, kind), _head()
    fresh.load_state_dict(model.state_dict())
    fresh_head.load_state_dict(head.state_dict())
    assert torch.equal(fresh(b['tokens'], b['pad_args']), want_logits), 'the inference forward of the trained model runs on stale derived weights'
    fresh.mark_trainable().train()
    got_loss = _backward(lambda: _head_loss(fresh, fresh_head, b), (fresh, fresh_head))
    got_grads = _grads((fresh, fresh_head))
    assert torch.equal(got_loss, want_loss) and set(got_grads) == set(want_grads) and len(want_grads) > 20
    for n in want_grads:
        assert torch.equal(got_grads[n], want_grads[n]), f'{n}: the trained model and a fresh one loaded from its state_dict differ'


@pytest.mark.parametrize('kind', KINDS)
def test_small_learning_rates_land(tmp_path, kind):
    """lr = 1e-5, 20 steps on a fixed batch.  Per tensor, the master's error against the float64 shadow, as a share of that shadow's total
    update, is at most 2 x the float32 shadow's -- two pipelines in one precision against one truth, the rule of
    tests/test_full_train_gpu.py -- with a floor of half an fp32 ulp of the weights per step; over all tensors together the bfloat16
    shadow (what torch.optim.AdamW on the model's own parameters does) is at least 10 x worse than the kernel."""
    steps, hp = 20, dict(lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    b = _batch(kind)
    model = _model(tmp_path, kind).mark_trainable().train()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    start = {n: p.detach().double().cpu() for n, p in named}
    shadows = {}
    for label, dt in (('f64', torch.float64), ('f32', torch.float32), ('bf16', torch.bfloat16)):
        ps = [torch.nn.Parameter(start[n].to(dt).clone()) for n, _ in named]         # (.to(float64) alone would alias `start`)
        shadows[label] = (ps, torch.optim.AdamW(ps, **hp))
    opt = esme.optim.AdamW([p for _, p in named], **hp)
    for _ in range(steps):
        _backward(lambda: _lm_loss(model, b), (model,))
        for ps, so in shadows.values():
            for q, (_, p) in zip(ps, named):
                q.grad = p.grad.detach().cpu().to(q.dtype)
            so.step()
        opt.step()
    sq = dict(kernel=0.0, f32=0.0, bf16=0.0, update=0.0)
    failures = []
    print()
    for i, (n, p) in enumerate(named):
        truth = shadows['f64'][0][i].detach()
        update = float((truth - start[n]).norm())
        master = opt.state[p]['master'].double().cpu()
        assert torch.equal(p.detach(), opt.state[p]['master'].to(torch.bfloat16)) and opt.state[p]['step'] == steps
        err = {'kernel': float((master - truth).norm()), 'f32': float((shadows['f32'][0][i].detach().double() - truth).norm()),
               'bf16': float((shadows['bf16'][0][i].detach().double() - truth).norm())}
        floor = steps * float(eb.half_ulp(start[n], 'fp32').norm())
        bar = max(2 * err['f32'], floor)
        print(f'[optim-train] {kind} {n:44s} share of the update lost: kernel {err["kernel"] / update:.2e}  fp32 shadow {err["f32"] / update:.2e}  '
              f'bf16 shadow {err["bf16"] / update:.3f}  bar {bar / update:.2e}')
        if err['kernel'] > bar:
            failures.append((n, err, bar))
        for k in err:
            sq[k] += err[k] ** 2
        sq['update'] += update ** 2
    share = {k: (sq[k] / sq['update']) ** 0.5 for k in ('kernel', 'f32', 'bf16')}
    print(f'[optim-train] {kind} all tensors: share of the float64 update lost: kernel {share["kernel"]:.2e}, fp32 shadow {share["f32"]:.2e}, bf16 shadow {share["bf16"]:.3f}')
    assert not failures, failures
    assert share['bf16'] >= 10 * share['kernel'], share


def test_lora_only_and_head_only(tmp_path):
    b = _batch('esm2')
    model, _ = golden_model(tmp_path, 'esm2')
    model.train()
    base = {n: p.detach().clone() for n, p in model.named_parameters() if '.lora_' not in n}
    lora = [p for n, p in model.named_parameters() if '.lora_' in n]
    assert lora and all(p.requires_grad for p in lora) and not any(p.requires_grad for n, p in model.named_parameters() if '.lora_' not in n)
    opt = esme.optim.AdamW(lora, lr=5e-3, weight_decay=0.0)
    losses = []
    for _ in range(6):
        losses.append(float(_backward(lambda: _lm_loss(model, b), (model,))))
        opt.step()
    print(f'\n[optim-train] LoRA only, six steps at lr 5e-3: loss {losses[0]:.4f} -> {losses[-1]:.4f}')
    assert losses[-1] < losses[0], losses
    assert all(torch.equal(p.detach(), base[n]) for n, p in model.named_parameters() if '.lora_' not in n)
    assert len(opt.state) == len(lora) and all(opt.state[p]['step'] == 6 for p in lora)
    # the head alone on a frozen backbone
    model.eval()
    head = _head()
    opt = esme.optim.AdamW(head.parameters(), lr=5e-3, max_grad_norm=10.0)
    losses = []
    for _ in range(6):
        losses.append(float(_backward(lambda: _head_loss(model, head, b, frozen=True), (head,))))
        opt.step()
    print(f'[optim-train] head only, six steps at lr 5e-3: loss {losses[0]:.4f} -> {losses[-1]:.4f}, last gradient norm {float(opt.last_grad_norm):.4f}')
    assert losses[-1] < losses[0], losses
    stepped = [p for p in head.parameters() if p in opt.state]
    assert stepped and all(opt.state[p]['step'] == 6 for p in stepped)       # (k.bias gets no gradient and is skipped)


def test_accumulate_over_four_micro_batches(tmp_path):
    """accumulate() after each of 4 backward passes, then one step, against float64 AdamW on the float64 mean of the same gradients.
    The first Adam step is invariant to the gradient's scale, so the moments are compared too: exp_avg = (1 - beta1) x mean."""
    kind = 'esm2'
    b = _batch(kind)
    model = _model(tmp_path, kind).mark_trainable(layers=[1]).train()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    start = {n: p.detach().double().cpu() for n, p in named}
    opt = esme.optim.AdamW([p for _, p in named], lr=1e-3, max_grad_norm=1e6)
    g = torch.Generator().manual_seed(3)
    total = {n: torch.zeros_like(s) for n, s in start.items()}
    for k in range(4):
        mask = (b['mask'].cpu() & (torch.rand(b['mask'].shape, generator=g) < 0.7)).to(DEV)
        _backward(lambda: _lm_loss(model, b, mask), ())
        for n, p in named:
            total[n] += p.grad.double().cpu()
        opt.accumulate()
        assert all(p.grad is None for _, p in named)
    opt.step()
    ps = [torch.nn.Parameter(start[n].clone()) for n, _ in named]
    for q, (n, _) in zip(ps, named):
        q.grad = total[n] / 4
    norm = float(torch.nn.utils.clip_grad_norm_(ps, 1e6))
    torch.optim.AdamW(ps, lr=1e-3).step()
    assert abs(float(opt.last_grad_norm) - norm) <= 1e-5 * norm              # the norm of the MEAN gradient
    for q, (n, p) in zip(ps, named):
        st = opt.state[p]
        mean = total[n] / 4
        # fp32 accumulation and arithmetic err by ~1e-7 relative; summing in bf16 would err by 2^-9, a sum instead of the mean by a factor 4
        assert float((st['exp_avg'].double().cpu() - 0.1 * mean).norm()) <= 1e-5 * float((0.1 * mean).norm()), n
        assert float((st['exp_avg_sq'].double().cpu() - 0.001 * mean * mean).norm()) <= 1e-5 * float((0.001 * mean * mean).norm()), n
        assert float((st['master'].double().cpu() - q.detach()).norm()) <= 1e-4 * float((q.detach() - start[n]).norm()), n
    _backward(lambda: _lm_loss(model, b), (model,))                          # without accumulate(), step() reads p.grad again
    opt.step()
    assert all(opt.state[p]['step'] == 2 for _, p in named)
    _backward(lambda: _lm_loss(model, b), (model,))
    opt.accumulate()
    _backward(lambda: _lm_loss(model, b), ())
    with pytest.raises(RuntimeError, match='not accumulated'):
        opt.step()


def _toy(seed=0, n=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(40 + 1000 * i, generator=g) * 0.05).to(torch.float32 if i == 1 else torch.bfloat16).to(DEV)) for i in range(n)]


def _toy_grads(params, seed):
    g = torch.Generator().manual_seed(seed)
    for p in params:
        p.grad = (5e-4 + 1e-3 * torch.randn(p.shape, generator=g)).to(p.dtype).to(DEV)


def test_exponential_lr_changes_the_next_step():
    params = _toy()
    shadow = [torch.nn.Parameter(p.detach().double().cpu()) for p in params]
    opt, ref = esme.optim.AdamW(params, lr=1e-2), torch.optim.AdamW(shadow, lr=1e-2)
    scheds = [torch.optim.lr_scheduler.ExponentialLR(o, gamma=0.1) for o in (opt, ref)]
    moves = []
    for k in range(2):
        _toy_grads(params, 20 + k)
        for p, q in zip(params, shadow):
            q.grad = p.grad.double().cpu()
        was = opt.state[params[4]]['master'].clone() if k else params[4].detach().float()
        opt.step()
        ref.step()
        moves.append(float((opt.state[params[4]]['master'] - was).abs().mean()))
        for s in scheds:
            s.step()
    assert opt.param_groups[0]['lr'] == pytest.approx(1e-4) and 0.02 < moves[1] / moves[0] < 0.5, moves      # the second step ran at lr 1e-3
    for p, q in zip(params, shadow):
        w = opt.state[p]['master'] if p.dtype == torch.bfloat16 else p.detach()
        assert float((w.double().cpu() - q.detach()).abs().max()) <= 1e-6       # (updates of 1e-2 and 1e-3; fp32 arithmetic errs by ~1e-8)


def test_a_resumed_run_continues_bit_equal():
    """Three steps, a checkpoint through torch.save, a new optimiser on copies of the parameters, two more steps on both: parameters,
    masters and moments bit-equal -- which they are not if the fp32 state comes back in the parameters' bfloat16."""
    a = _toy(seed=1)
    opt_a = esme.optim.AdamW([{'params': a[:2]}, {'params': a[2:], 'lr': 1e-5}], lr=1e-4, max_grad_norm=0.05)
    for k in range(3):
        _toy_grads(a, 30 + k)
        opt_a.step()
    f = io.BytesIO()
    torch.save(opt_a.state_dict(), f)
    f.seek(0)
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    opt_b = esme.optim.AdamW([{'params': b[:2]}, {'params': b[2:]}], lr=1.0, max_grad_norm=0.05)
    opt_b.load_state_dict(torch.load(f))
    with warnings.catch_warnings():
        warnings.simplefilter('error')                                        # no re-seed on either side
        for k in range(2):
            _toy_grads(a, 40 + k)
            _toy_grads(b, 40 + k)
            opt_a.step()
            if k:
                opt_b.accumulate()                                            # (one accumulated micro-batch is the same step)
            opt_b.step()
    for p, q in zip(a, b):
        assert torch.equal(p.detach(), q.detach())
        sa, sb = opt_a.state[p], opt_b.state[q]
        assert sa['step'] == sb['step'] == 5 and set(sa) == set(sb)
        for key in ('master', 'exp_avg', 'exp_avg_sq'):
            if key in sa:
                assert sb[key].dtype == torch.float32 and torch.equal(sa[key], sb[key]), key
    assert any(not torch.equal(opt_a.state[p]['master'], p.detach().float()) for p in a if p.dtype == torch.bfloat16)     # the masters carry more than bf16


def test_a_foreign_write_reseeds_the_master_with_a_warning():
    params = _toy(seed=2, n=3)
    opt = esme.optim.AdamW(params, lr=1e-4)
    _toy_grads(params, 50)
    opt.step()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        _toy_grads(params, 51)
        opt.step()                                                            # our own writes do not count
    new = (torch.randn(params[2].shape, generator=torch.Generator().manual_seed(9)) * 0.05).to(torch.bfloat16).to(DEV)
    with torch.no_grad():
        params[2].copy_(new)                                                  # e.g. load_state_dict or load_lora
    old_master = opt.state[params[0]]['master'].clone()
    _toy_grads(params, 52)
    with pytest.warns(RuntimeWarning, match='1 parameter.*re-seeded'):
        opt.step()
    assert float((opt.state[params[2]]['master'] - new.float()).abs().max()) <= 2e-4         # one step of at most ~lr away from the written values
    assert float((opt.state[params[0]]['master'] - old_master).abs().max()) <= 2e-4 and opt.state[params[2]]['step'] == 3
    assert torch.equal(params[2].detach(), opt.state[params[2]]['master'].to(torch.bfloat16))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        _toy_grads(params, 53)
        opt.step()
