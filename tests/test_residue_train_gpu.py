"""Per-residue fine-tuning end to end on the device: a two-layer ESM-2 (E = 64, H = 2) and a two-layer ESM-C of esme.synthetic, each
with LoRA adapters (rank 4 on query / value / output) and a trainable ResidueHead of three labels, on six packed sequences.

 - ResidueModel.loss_trainable is head.loss on forward_trainable(logits=False, layers=...), bit for bit, with and without layers=[0]
   and checkpoint_layers=True.
 - The adapters' gradients against a reference route: the float64 dX of tests/linear_xent_bounds.py's restatement, rounded to bfloat16,
   put into rep.backward(...).  The criterion of tests/test_taps_train_gpu.py for gradients through a head: per tensor the relative
   Frobenius error is within 2 x the error of the same data flow in bfloat16 torch ops (F.linear -> F.cross_entropy on the same
   representation) against that reference.  The head's own gradients are held to the kernel's bound (tests/test_linear_xent_gpu.py).
 - model.masked_lm_loss against esme.cross_entropy(model.forward_trainable(...), tokens, mask): the two losses agree within the kernel's
   bound for its loss plus the roundings of the existing route -- its logits and log-probabilities rounded to bfloat16 (a logit moved
   by d moves a row's loss by at most 2 d) and its bfloat16 result; 2-D tokens agree with packed within the fp32 summation bound.
 - Twenty steps of tools/residue_finetune.py's loop lower the loss (the last below the first; no magnitude is fixed).
The measured values are printed (profiles/residue_train_parity.txt keeps a run's output)."""
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

import error_bounds as eb
import linear_xent_bounds as LB
from golden_util import rel_fro
from test_lora_gpu import tiny

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KINDS = ('esm2', 'esmc')
LENGTHS = (1, 2, 63, 64, 65, 129)                 # residues per sequence (+ <cls> and <eos>)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('residue_finetune', os.path.join(ROOT, 'tools', 'residue_finetune.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _net(tmp_path, kind, layers=None, seed=3):
    from esme.head import ResidueHead
    from esme.trainer import ResidueModel
    model = tiny(tmp_path, kind, 2, 64, 2, seed).add_lora(rank=4, alpha=4, layers=('query', 'value', 'output'))
    model.mark_only_lora_as_trainable()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if '.lora_B' in n:                                                    # (B starts at zero: give the adapters an effect and A a gradient)
                p.copy_((0.05 * torch.randn(p.shape, generator=g)).to(p.dtype))
    torch.manual_seed(seed)
    head = ResidueHead(64 * (1 + len(layers or ())), 3).to(DEV).requires_grad_(True)
    return ResidueModel(model.train(), head, layers=layers)


def _batch(seed=5):
    from esme.data import ResidueLabeledDataset
    T = _tool()
    g = torch.Generator().manual_seed(seed)
    seqs = [''.join(T.RESIDUES[i] for i in torch.randint(0, len(T.RESIDUES), (n,), generator=g).tolist()) for n in LENGTHS]
    labels = [[T.CLASS_OF[c] for c in s[T.SHIFT:]] + [-1] * min(T.SHIFT, len(s)) for s in seqs]
    item = ResidueLabeledDataset(seqs, labels, 10_000, shuffle=False)[0]
    return T.batch_to(item, DEV)


def _grads(module):
    return {n: p.grad.clone() for n, p in module.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('kind', KINDS)
def test_loss_trainable_is_the_head_loss_on_the_trainable_representation(tmp_path, kind):
    token, pad_args, label = _batch()
    assert token.numel() == sum(LENGTHS) + 2 * len(LENGTHS) and int((label >= 0).sum()) == sum(max(n - 2, 0) for n in LENGTHS)
    for layers in (None, [0]):
        net = _net(tmp_path, kind, layers)
        results = []
        for ckpt in (False, True):
            net.zero_grad(set_to_none=True)
            loss = net.loss_trainable(token, pad_args, label, checkpoint_layers=ckpt)
            assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.grad_fn is not None
            loss.backward()
            results.append((loss.detach().clone(), _grads(net)))
            net.zero_grad(set_to_none=True)
            rep = net.plm.forward_trainable(token, pad_args, logits=False, layers=layers, checkpoint_layers=ckpt)
            assert rep.shape == (token.numel(), net.width)
            direct = net.head.loss(rep, label)
            direct.backward()
            assert torch.equal(direct.detach(), results[-1][0])
            again = _grads(net)
            assert set(again) == set(results[-1][1]) and all(torch.equal(again[n], results[-1][1][n]) for n in again)
        (l0, g0), (l1, g1) = results
        assert torch.equal(l0, l1) and set(g0) == set(g1) and len(g0) >= 12 + 2          # checkpointing changes no bit
        for n in g0:
            assert torch.equal(g0[n], g1[n]), n
        net.eval()                                                                # the inference route (the fused forward runs adapters in eval() only)
        logits = net(token, pad_args)
        assert logits.shape == (token.numel(), 3) and logits.dtype == torch.bfloat16 and not logits.requires_grad
        assert torch.equal(net.predict(token, pad_args), logits.argmax(-1))
        net.train()
    frozen = _net(tmp_path, kind)
    for p in frozen.plm.parameters():
        p.requires_grad_(False)
    assert not frozen.backbone_trains()
    frozen.plm.eval()                                                             # (frozen adapters run in the fused forward, which serves eval() only)
    loss = frozen.loss_trainable(token, pad_args, label)                          # a frozen backbone: forward_representation, only the head trains
    loss.backward()
    assert set(_grads(frozen)) == {'head.classifier.weight', 'head.classifier.bias'}
    assert bool(torch.isfinite(loss)) and float(loss.detach()) > 0


@pytest.mark.parametrize('kind', KINDS)
def test_backbone_gradients_against_the_float64_head(tmp_path, kind):
    token, pad_args, label = _batch()
    net = _net(tmp_path, kind, [0])
    lin = net.head.classifier
    w, b = lin.weight.detach(), lin.bias.detach()
    one = torch.ones(1, dtype=torch.float32, device=DEV)

    def backbone_grads(push):
        net.zero_grad(set_to_none=True)
        rep = net.plm.forward_trainable(token, pad_args, logits=False, layers=[0])
        push(rep)
        return rep.detach(), _grads(net.plm)
    rep, ours = backbone_grads(lambda rep: net.head.loss(rep, label).backward())
    head_grads = _grads(net.head)
    ref = LB.reference(rep, w, b, label, None, one, True)
    bnd = LB.bound(rep, w, b, label, None, one, True)
    _, want = backbone_grads(lambda rep: rep.backward(ref['dx'].to(torch.bfloat16)))
    _, flow = backbone_grads(lambda rep: F.cross_entropy(F.linear(rep, lin.weight, lin.bias), label, ignore_index=-100).backward())
    assert set(ours) == set(want) == set(flow) and len(ours) >= 12
    failures = []
    print()
    for n in sorted(ours):
        bar = 2 * rel_fro(flow[n].float().cpu(), want[n].double().cpu())
        err = rel_fro(ours[n].float().cpu(), want[n].double().cpu())
        print(f'[residue-train] {kind} {n:52s} error {err:.5f}  bar {bar:.5f}  ({err / bar if bar else float("inf"):.2f})')
        if err > bar:
            failures.append((n, err, bar))
    assert not failures, failures
    got = dict(dw=head_grads['classifier.weight'], db=head_grads['classifier.bias'])
    worst = LB.worst_of(got, ref, bnd, ('dw', 'db'))
    print(f'[residue-train] {kind} head gradients: worst err / bound {worst}')
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize('kind', KINDS)
def test_masked_lm_loss_against_the_materialised_route(tmp_path, kind):
    import esme
    from esme.alphabet import mask_tokens
    model = tiny(tmp_path, kind, 2, 64, 2, 3).add_lora(rank=4, alpha=4, layers=('query', 'value', 'output'))
    model.mark_only_lora_as_trainable().mark_lmhead(True)
    model.train()
    token, pad_args, _ = _batch()
    torch.manual_seed(1)
    masked, mask = mask_tokens(token.cpu(), 0.3, 0.1, alphabet=model.alphabet)
    masked, mask = masked.to(DEV), mask.to(DEV)
    assert int(mask.sum()) > 20
    model.zero_grad(set_to_none=True)
    ours = model.masked_lm_loss(masked, pad_args, token, mask)
    assert ours.dtype == torch.float32 and ours.dim() == 0
    ours.backward()
    g_ours = _grads(model)
    model.zero_grad(set_to_none=True)
    theirs = esme.cross_entropy(model.forward_trainable(masked, pad_args), token, mask, alphabet=model.alphabet)
    theirs.backward()
    g_theirs = _grads(model)
    assert set(g_ours) == set(g_theirs) and 'lm_head.final.weight' in g_ours and any('.lora_A' in n for n in g_ours)
    with torch.no_grad():
        h = model.lm_head.features_trainable(model.forward_trainable(masked, pad_args, logits=False))
    lin = model.lm_head.final
    labels = torch.where(mask & (token != model.alphabet.padding_idx), token, torch.full_like(token, -100))
    one = torch.ones(1, dtype=torch.float32, device=DEV)
    args = (h, lin.weight.detach(), lin.bias.detach(), labels, None, one, True)
    ref, bnd = LB.reference(*args), LB.bound(*args)
    assert abs(float(ours.detach()) - float(ref['loss'])) <= float(bnd['loss'])            # the fused route within the kernel's own bound
    # the existing route: logits rounded to bfloat16 (a logit moved by d moves a row's loss by at most 2 d), log-probabilities rounded to
    # bfloat16, a bfloat16 result
    kept = LB._kept(labels, lin.weight.shape[0])
    z = h.double() @ lin.weight.detach().double().T + lin.bias.detach().double()
    e_z = LB.gamma(h.shape[1] + 1) * (h.double().abs() @ lin.weight.detach().double().abs().T + lin.bias.detach().double().abs())
    d = (eb.half_ulp(z.abs() + e_z, 'bf16') + e_z).max(dim=1).values
    rows = 2 * d + eb.half_ulp(ref['loss_rows'].abs() + 2 * d, 'bf16')
    existing = float(rows[kept].sum() / kept.sum())
    existing += float(eb.half_ulp(ref['loss'].abs() + existing, 'bf16'))
    diff = abs(float(ours.detach()) - float(theirs.detach()))
    print(f'\n[residue-train] {kind} masked-LM loss: fused {float(ours.detach()):.6f}  materialised {float(theirs.detach()):.6f}  float64 {float(ref["loss"]):.6f}  '
          f'|difference| {diff:.3e}  bound {float(bnd["loss"]) + existing:.3e}')
    assert diff <= float(bnd['loss']) + existing
    for n in sorted(g_ours):                                                      # the gradients of the two routes, printed (no bar: neither is the truth)
        err = rel_fro(g_ours[n].float().cpu(), g_theirs[n].double().cpu())
        print(f'[residue-train] {kind} {n:52s} fused against materialised {err:.5f}')
        assert bool(torch.isfinite(g_ours[n].float()).all()), n
    # 2-D tokens: the rows' losses are the packed ones, summed in another order
    cu = pad_args[0].tolist()
    pad = model.alphabet.padding_idx
    shape = (len(cu) - 1, pad_args[1])
    tok2d, msk2d = torch.full(shape, pad, dtype=torch.int64, device=DEV), torch.full(shape, pad, dtype=torch.int64, device=DEV)
    m2d = torch.zeros(shape, dtype=torch.bool, device=DEV)
    for i, (a, e) in enumerate(zip(cu[:-1], cu[1:])):
        tok2d[i, :e - a], msk2d[i, :e - a], m2d[i, :e - a] = token[a:e], masked[a:e], mask[a:e]
    m2d[0, -1] = True                                                             # a selected <pad> position is ignored, as in esme.cross_entropy
    two_d = model.masked_lm_loss(msk2d, None, tok2d, m2d)
    print(f'[residue-train] {kind} masked-LM loss, 2-D tokens {float(two_d.detach()):.6f}  packed {float(ours.detach()):.6f}')
    assert abs(float(two_d.detach()) - float(ours.detach())) <= 2 * float(bnd['loss'])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')                                       # the loss and its backward leave the host alone
    try:
        model.masked_lm_loss(masked, pad_args, token, mask).backward()
    finally:
        torch.cuda.set_sync_debug_mode('default')


def test_twenty_steps_of_the_tool_lower_the_loss(tmp_path):
    import esme
    from esme.data import ResidueLabeledDataset
    T = _tool()
    net = _net(tmp_path, 'esm2', [0])
    opt = esme.optim.AdamW(net.param_groups(1e-3, 1e-2), weight_decay=0.0)
    data = ResidueLabeledDataset(*T.make_task(24, seed=0, lo=20, hi=60), 600, shuffle=True, random_state=0)
    batches = [data[i] for i in range(len(data))]
    assert len(batches) >= 2
    lines = []
    losses = T.train_steps(net, opt, batches, DEV, 20, log=lines.append)
    print('\n[residue-train] ' + '  '.join(f'{l:.4f}' for l in losses))
    assert len(losses) == len(lines) == 20 and all(torch.isfinite(torch.tensor(losses)))
    assert losses[-1] < losses[0]
    acc = T.accuracy(net, batches, DEV)
    print(f'[residue-train] accuracy after 20 steps: {acc:.4f}')
    assert 0.0 <= acc <= 1.0
