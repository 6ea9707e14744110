"""Supervised fine-tuning end to end on the device: esme.data.LabeledDataset -> esme.trainer.RegressionModel (a fixture backbone with
LoRA adapters of rank 4, the raw output of layer 1 next to the final representation, a BinaryLearnedAggregation head of width 2 E) ->
F.mse_loss(reduction='sum') -> esme.optim.AdamW with the reference's two learning-rate groups.  64 synthetic sequences of 20 .. 60
residues are labelled with their tryptophan fraction; with fixed seeds and deterministic kernels the mean training loss of the last
five of 30 steps must lie strictly below that of the first five, and the inference route (`model.eval()`, RegressionModel.forward)
must see the trained adapters.  Then the heads on a tapped representation (ClsHead's backward is esme_hip_segment_mean_bwd) and the
reductions of the reference."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import esme
from esme.data import LabeledDataset
from esme.head import ClsHead
from esme.pooling import BinaryLearnedAggregation
from esme.trainer import RegressionModel, spearman
from test_lora_gpu import tiny

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RESIDUES = 'ACDEFGHIKLMNPQRSTVWY'


def _data(n=64, seed=7):
    rng = np.random.Generator(np.random.PCG64(seed))
    seqs = []
    for _ in range(n):
        p_w = rng.uniform(0.0, 0.3)                                        # (the share of tryptophan varies: there is something to learn)
        length = int(rng.integers(20, 61))
        seqs.append(''.join('W' if rng.uniform() < p_w else RESIDUES[int(rng.integers(0, 18))] for _ in range(length)))
    return seqs, [s.count('W') / len(s) for s in seqs]


def _net(tmp_path, head='attention', layers=(1,), lora=True):
    torch.manual_seed(0)
    model = tiny(tmp_path, 'esm2', 3, 128, 2, 41)
    for p in model.parameters():
        p.requires_grad_(False)
    if lora:
        model.add_lora(rank=4, alpha=4, layers=('query', 'value', 'output'))
        model.mark_only_lora_as_trainable()
    width = model.embed_dim * (1 + len(layers))
    h = BinaryLearnedAggregation(2, width) if head == 'attention' else ClsHead(width, hidden_dim=256)
    return RegressionModel(model, h.to(DEV).requires_grad_(True), layers=list(layers))


def _to(batch):
    return batch['token'].to(DEV), (batch['cu_lens'].to(DEV), int(batch['max_len'])), batch['label'].to(DEV)


def test_thirty_steps_lower_the_loss_and_reach_the_inference_route(tmp_path):
    seqs, labels = _data()
    assert len(seqs) == 64 and min(map(len, seqs)) >= 20 and max(map(len, seqs)) <= 60
    data = LabeledDataset(seqs, labels, token_per_batch=1400, shuffle=True, random_state=0)
    assert len(data) >= 2
    net = _net(tmp_path)
    groups = net.param_groups(lr=1e-3, lr_head=2e-3)
    assert [g['lr'] for g in groups] == [2e-3, 1e-3] and all('.lora_' in n for n, p in net.plm.named_parameters() if p.requires_grad)
    opt = esme.optim.AdamW(groups, weight_decay=0.0)
    token0, pad0, _ = _to(data[0])
    net.eval()
    before, rep_before = net(token0, pad0).clone(), net.plm.forward_representation(token0, pad0, layers=[1]).clone()
    assert before.shape == (len(data.sampler[0]),) and before.grad_fn is None
    net.train()
    losses, step = [], 0
    while step < 30:
        for batch in data.to_dataloader():
            token, pad_args, label = _to(batch)
            net.zero_grad(set_to_none=True)
            y = net.forward_trainable(token, pad_args)
            assert y.shape == label.shape and y.grad_fn is not None
            loss = F.mse_loss(y.float(), label, reduction='sum')
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            step += 1
            if step == 30:
                break
    first, last = sum(losses[:5]) / 5, sum(losses[-5:]) / 5
    print(f'\n[supervised] 30 AdamW steps: mean loss of the first five {first:.5f}, of the last five {last:.5f}')
    assert last < first, losses
    net.eval()
    after, rep_after = net(token0, pad0), net.plm.forward_representation(token0, pad0, layers=[1])
    assert not torch.equal(after, before)
    assert not torch.equal(rep_after, rep_before)                          # the fused inference forward runs the trained adapters
    rho = spearman(after.float().cpu(), data[0]['label'])
    print(f'[supervised] Spearman on the first training batch after training: {rho:.3f}')


@pytest.mark.parametrize('head', ('attention', 'mean'))
def test_heads_take_the_tapped_representation(tmp_path, head):
    seqs, labels = _data(12, seed=3)
    net = _net(tmp_path, head=head, layers=(0, 2)).train()
    assert net.width == 3 * 128
    token, pad_args, label = _to(LabeledDataset(seqs, labels, token_per_batch=4096, shuffle=False)[0])
    y = net.forward_trainable(token, pad_args)
    assert y.shape == (12,) and y.grad_fn is not None
    F.mse_loss(y.float(), label, reduction='sum').backward()
    for n, p in net.named_parameters():
        if p.requires_grad and not n.endswith('attn.k.bias'):
            assert p.grad is not None and bool(torch.isfinite(p.grad.float()).all()), n
    assert any('.lora_B.' in n and bool(p.grad.any()) for n, p in net.plm.named_parameters() if p.grad is not None)
    net.eval()
    z = net(token, pad_args)
    assert z.shape == (12,) and z.grad_fn is None and bool(torch.isfinite(z.float()).all())


def test_frozen_backbone_and_reductions(tmp_path):
    seqs, labels = _data(6, seed=5)
    batch = LabeledDataset(seqs, labels, token_per_batch=4096, shuffle=False)[0]
    token, pad_args, label = _to(batch)
    indices = batch['indices'].to(DEV)
    net = _net(tmp_path, lora=False)
    assert not net.backbone_trains() and len(net.param_groups()) == 1
    y = net.forward_trainable(token, pad_args)                             # the fused forward under no_grad, the head with a backward
    y.float().sum().backward()
    assert all(p.grad is None for p in net.plm.parameters()) and net.head.linear.weight.grad is not None
    for reduction in ('mean', 'sum'):
        lin = torch.nn.Linear(256, 1).to(DEV).to(torch.bfloat16)
        red = RegressionModel(net.plm, lin, layers=[1], reduction=reduction)
        out = red(token, pad_args, pad_output=True, pad_indices=indices)
        rep = net.plm.forward_representation(token, pad_args, pad_output=True, pad_indices=indices, layers=[1])
        want = lin(rep.mean(dim=1) if reduction == 'mean' else rep.sum(dim=1))
        assert out.shape == (6, 1) and torch.equal(out, want.detach())
        with pytest.raises(ValueError, match='pad_output=True'):
            red(token, pad_args)
    with pytest.raises(ValueError, match='Unknown reduction'):
        RegressionModel(net.plm, net.head, reduction='max')
