"""Fine-tuning the task heads on the device: forward_trainable of LearnedAggregation, BinaryLearnedAggregation and ClsHead.

Gradients are judged against float64 autograd through the reference's data flow, restated here with attn_pool_bounds.reference_pool as
the model: the key projection with its bias over every row, a softmax per (class token, head) over each sequence's rows, the weights
applied to the raw embedding, then the MLP -- on the same bf16-valued parameters.  The bar per tensor, in relative Frobenius error, is
2 x the error that the same data flow run in bf16 torch ops makes against that truth (computed here, not taken from the code under
test): two independent bf16 pipelines against one truth make errors of that size each, the rule tests/test_lora_train_gpu.py uses.
Seed and scales were chosen on the CPU so that every bar lies in (1e-3, 0.1), which is asserted.  The measured values are printed per
tensor (profiles/head_train_parity.txt keeps a run's output).  Then forward_trainable against forward, and a short training run of the
tiny ESM-2 fixture with the g13 adapters and a BinaryLearnedAggregation head."""
import math

import pytest
import torch
import torch.nn.functional as F

import attn_pool_bounds as apb
from golden_util import rel_fro

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LENGTHS = (1, 40, 64, 65, 130)
E, H = 128, 4
FACTOR = 2.0
_SHARED = {}


def _heads():
    from esme.head import ClsHead
    from esme.pooling import BinaryLearnedAggregation, LearnedAggregation
    return {'LearnedAggregation': lambda: LearnedAggregation(3, H, E), 'BinaryLearnedAggregation': lambda: BinaryLearnedAggregation(H, E),
            'ClsHead': lambda: ClsHead(E, 2, 256)}


KINDS = ('LearnedAggregation', 'BinaryLearnedAggregation', 'ClsHead')


def make_head(kind, seed=5):
    """The head with seeded bf16 parameters of scale 1 / sqrt(fan-in) (class tokens and biases of scale 1 and 0.1)."""
    head = _heads()[kind]()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in head.named_parameters():
            scale = 0.1 if p.dim() == 1 else (1.0 if n.endswith('cls') else 1.0 / math.sqrt(p.shape[-1]))
            p.copy_((torch.randn(p.shape, generator=g) * scale).to(p.dtype))
    return head


def make_batch(seed=5):
    g = torch.Generator().manual_seed(seed)
    embed = torch.randn(sum(LENGTHS), E, generator=g).to(torch.bfloat16)
    cu = torch.tensor([0] + list(torch.tensor(LENGTHS).cumsum(0)), dtype=torch.int32)
    return embed, cu


def _labels(shape, seed=12):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def flow(kind, P, x, cu):
    """The reference's data flow in torch ops of x's dtype on the parameters P (name -> tensor of that dtype)."""
    cl = [int(c) for c in cu]
    if kind == 'ClsHead':
        pooled = torch.stack([x[a:b].mean(0) for a, b in zip(cl[:-1], cl[1:])])
        return F.linear(F.relu(F.linear(pooled, P['head.0.weight'], P['head.0.bias'])), P['head.2.weight'], P['head.2.bias']).squeeze(-1)
    cls, T = P['attn.cls'], x.shape[0]
    C, d = cls.shape[0], E // H
    k = F.linear(x, P['attn.k.weight'], P['attn.k.bias']).view(T, H, d)              # the key projection, with its bias, over every row
    scores = torch.einsum('thd,chd->tch', k, cls.view(C, H, d)) / math.sqrt(d)
    pooled = torch.stack([torch.einsum('tch,thd->chd', torch.softmax(scores[a:b], dim=0), x[a:b].view(-1, H, d)).reshape(C, E)
                          for a, b in zip(cl[:-1], cl[1:])])
    y = F.linear(F.relu(F.linear(pooled, P['linear.weight'], P['linear.bias'])), P['final.weight'], P['final.bias']).squeeze(1)
    return y.squeeze(-1) if kind == 'BinaryLearnedAggregation' else y


def run_flow(kind, head, embed, cu, dtype, labels=None):
    """(output, {name: gradient}) of the data flow in `dtype` with a sum-reduced MSE loss; 'embed' names the embedding's gradient."""
    P = {n: p.detach().to(dtype).clone().requires_grad_() for n, p in head.named_parameters()}
    x = embed.detach().to(dtype).clone().requires_grad_()
    y = flow(kind, P, x, cu)
    if labels is None:
        return y.detach(), {}
    acc = torch.float64 if dtype == torch.float64 else torch.float32
    F.mse_loss(y.to(acc), labels.to(y.device).to(acc), reduction='sum').backward()
    return y.detach(), dict({n: p.grad for n, p in P.items()}, embed=x.grad)


def truth_and_bars(kind, device='cpu'):
    """float64 truth (output and gradients) and the bar of every tensor: FACTOR x the bf16 torch pipeline's error against it."""
    head = make_head(kind).to(device)
    embed, cu = make_batch()
    embed = embed.to(device)
    labels = _labels(run_flow(kind, head, embed, cu, torch.float64)[0].shape)
    y64, g64 = run_flow(kind, head, embed, cu, torch.float64, labels=labels)
    y16, g16 = run_flow(kind, head, embed, cu, torch.bfloat16, labels=labels)
    bars = {n: FACTOR * rel_fro(g16[n].double().cpu(), g64[n].cpu()) for n in g64 if not n.endswith('k.bias')}
    return dict(head=head, embed=embed, cu=cu, labels=labels, y64=y64, g64=g64, bars=bars, out_bar=FACTOR * rel_fro(y16.double().cpu(), y64.cpu()))


def _case(kind):
    if kind not in _SHARED:
        _SHARED[kind] = truth_and_bars(kind, DEV)
    return _SHARED[kind]


def _call(head, kind, fn, embed, cu):
    return getattr(head, fn)(embed, cu.to(embed.device)) if kind == 'ClsHead' else getattr(head, fn)(embed, (cu.to(embed.device), max(LENGTHS)))


def test_the_restated_data_flow_is_reference_pool():
    head = make_head('LearnedAggregation')
    embed, cu = make_batch()
    a = head.attn
    ref, _ = apb.reference_pool(embed, cu, a.cls, a.k.weight, a.k.bias, H)
    P = {n: p.detach().double() for n, p in head.named_parameters()}
    pooled = ref.to(torch.float64)
    want = F.linear(F.relu(F.linear(pooled, P['linear.weight'], P['linear.bias'])), P['final.weight'], P['final.bias']).squeeze(1)
    assert torch.allclose(flow('LearnedAggregation', P, embed.double(), cu), want, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize('kind', KINDS)
def test_gradients_against_float64_autograd(kind):
    c = _case(kind)
    head = make_head(kind).to(DEV).requires_grad_(True)
    head.train()
    embed = c['embed'].clone().requires_grad_()
    y = _call(head, kind, 'forward_trainable', embed, c['cu'])
    assert y.grad_fn is not None and y.dtype == torch.bfloat16 and y.shape == c['y64'].shape
    F.mse_loss(y.float(), c['labels'].to(DEV), reduction='sum').backward()
    grads = dict({n: p.grad for n, p in head.named_parameters()}, embed=embed.grad)
    failures = []
    print()
    for n, bar in c['bars'].items():
        assert 1e-3 < bar < 0.1, f'{kind} {n}: the bar {bar:.3e} is outside (1e-3, 0.1)'
        g = grads[n]
        assert g is not None and bool(torch.isfinite(g.float()).all()) and g.dtype == torch.bfloat16, n
        err = rel_fro(g.double().cpu(), c['g64'][n].cpu())
        print(f'[head-train] {kind:26s} {n:16s} error {err:.5f}  bar {bar:.5f}  ({err / bar:.2f})')
        if err > bar:
            failures.append((n, err, bar))
    if kind != 'ClsHead':
        assert head.attn.k.bias.grad is None                                   # the bias cancels in the softmax: no gradient is made for it
    assert not failures, failures


@pytest.mark.parametrize('kind', KINDS)
def test_forward_trainable_equals_forward(kind):
    c = _case(kind)
    head = make_head(kind).to(DEV)
    for mode in (head.train, head.eval):                                       # the same in train() and eval()
        mode()
        with torch.no_grad():
            ft = _call(head, kind, 'forward_trainable', c['embed'], c['cu'])
            fw = _call(head, kind, 'forward', c['embed'], c['cu'])
        assert ft.shape == fw.shape and ft.dtype == fw.dtype
        dist = rel_fro(ft.double().cpu(), fw.double().cpu())
        print(f'\n[head-train] {kind} forward_trainable against forward: {dist:.5f}  bar {c["out_bar"]:.5f}')
        assert dist <= c['out_bar'], (kind, dist, c['out_bar'])
    x32 = c['embed'].float().requires_grad_()                                   # a float32 embedding that requires grad is served too
    y32 = _call(head.requires_grad_(True), kind, 'forward_trainable', x32, c['cu'])
    assert y32.dtype == torch.float32 and y32.shape == fw.shape
    y32.square().sum().backward()
    assert x32.grad is not None and x32.grad.dtype == torch.float32 and bool(torch.isfinite(x32.grad).all()) and bool(x32.grad.any())
    assert rel_fro(y32.detach().double().cpu(), c['y64'].cpu()) <= c['out_bar']


def _lens_labels(cu, max_len):
    return ((cu[1:] - cu[:-1]).float() / max_len).to(DEV)                       # a fixed function of the sequence length


def _train(model, head, tokens, pad_args, labels, frozen, steps=10):
    params = list(head.parameters()) + ([] if frozen else [p for p in model.parameters() if p.requires_grad])
    opt = torch.optim.Adam(params, lr=5e-3)
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        if frozen:
            with torch.no_grad():
                rep = model.forward_representation(tokens, pad_args)
        else:
            rep = model.forward_trainable(tokens, pad_args, logits=False)
        loss = F.mse_loss(head.forward_trainable(rep, pad_args).float(), labels, reduction='sum')
        loss.backward()
        losses.append(float(loss.detach()))
        if len(losses) < steps:
            opt.step()
    return losses, rep.detach()


def test_end_to_end_training(tmp_path, monkeypatch):
    from esme import _hip_attn_pool_bwd
    from esme.pooling import BinaryLearnedAggregation
    from test_lora_gpu import golden_model
    model, g13 = golden_model(tmp_path, 'esm2')
    tokens, pad_args = g13['esm2_tokens'].to(DEV), (g13['cu_lens'].to(DEV), int(g13['max_len']))
    labels = _lens_labels(pad_args[0], pad_args[1])
    asked, kernel = [], _hip_attn_pool_bwd.attn_pool_bwd
    monkeypatch.setattr(_hip_attn_pool_bwd, 'attn_pool_bwd', lambda *a, need_dx=True, **kw: (asked.append(need_dx), kernel(*a, need_dx=need_dx, **kw))[1])
    assert model.embed_dim == E

    # head and adapters
    head = make_head('BinaryLearnedAggregation', seed=21).to(DEV).requires_grad_(True)
    model.train()
    losses, rep = _train(model, head, tokens, pad_args, labels, frozen=False)
    print(f'\n[head-train] ten Adam steps, head + adapters: loss {losses[0]:.4f} -> {losses[-1]:.4f}')
    assert losses[-1] < losses[0], losses
    assert asked and all(asked)                                                 # the adapters need the embedding gradient
    for n, p in model.named_parameters():
        if '.lora_' in n:
            assert p.grad is not None and bool(torch.isfinite(p.grad.float()).all()) and bool(p.grad.any()), n
        else:
            assert p.grad is None, f'{n}: a base weight got a gradient'
    for n, p in head.named_parameters():
        if n.endswith('k.bias'):
            assert p.grad is None
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad.float()).all()) and bool(p.grad.any()), n

    # the backbone frozen: the head alone, and the kernel is never asked for dx
    del asked[:]
    model.eval()
    head2 = make_head('BinaryLearnedAggregation', seed=21).to(DEV).requires_grad_(True)
    losses2, rep2 = _train(model, head2, tokens, pad_args, labels, frozen=True)
    print(f'[head-train] ten Adam steps, head alone: loss {losses2[0]:.4f} -> {losses2[-1]:.4f}')
    assert losses2[-1] < losses2[0], losses2
    assert asked and not any(asked)

    # the trained head at inference, and through a state_dict
    head2.eval()
    with torch.no_grad():
        ft, fw = head2.forward_trainable(rep2, pad_args), head2(rep2, pad_args)
    y64 = run_flow('BinaryLearnedAggregation', head2, rep2, pad_args[0], torch.float64)[0]
    y16 = run_flow('BinaryLearnedAggregation', head2, rep2, pad_args[0], torch.bfloat16)[0]
    bar = FACTOR * rel_fro(y16.double().cpu(), y64.cpu())
    dist = rel_fro(ft.double().cpu(), fw.double().cpu())
    print(f'[head-train] trained head, forward_trainable against forward: {dist:.5f}  bar {bar:.5f}')
    assert dist <= bar, (dist, bar)
    fresh = BinaryLearnedAggregation(H, E)
    fresh.load_state_dict({k: v.cpu() for k, v in head2.state_dict().items()})
    assert all(not p.requires_grad for p in fresh.parameters())
    assert torch.equal(fresh.to(DEV).eval()(rep2, pad_args), fw)
