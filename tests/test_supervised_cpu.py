"""Supervised fine-tuning without a GPU: esme.data.LabeledDataset against what the reference's class yields
(tests/golden/g16_labeled_dataset.json, made by tests/golden/make_golden_labeled_dataset.py: two token budgets, shuffle off and on
with a seed, truncate_len unset and set, sequences of 1 .. 40 residues); the argument checks of forward_trainable(layers=...), which
raise before the first kernel call; and the host side of esme.trainer (RegressionModel's groups and reductions, Spearman's rho)."""
import json
import os

import pytest
import torch

from esme import ESM, synthetic as syn
from esme.data import LabeledDataset, TokenSizeBatchSampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'g16_labeled_dataset.json')
_G = {}


def _golden():
    if not _G:
        with open(FIXTURE) as f:
            _G.update(json.load(f))
    return _G


def _ids():
    return [f"budget{c['token_per_batch']}-{'shuffle' if c['shuffle'] else 'ordered'}-trunc{c['truncate_len']}" for c in _golden()['cases']]


def test_the_fixture_covers_the_issue():
    g = _golden()
    assert sorted(len(s) for s in g['seqs']) == list(range(1, 41)) and len(g['labels']) == 40
    cases = {(c['token_per_batch'], c['shuffle'], c['truncate_len']) for c in g['cases']}
    assert len({b for b, _, _ in cases}) == 2 and len(cases) == 8
    assert {s for _, s, _ in cases} == {True, False} and {t is None for _, _, t in cases} == {True, False}
    for c in g['cases']:
        assert sorted(i for it in c['items'] for i in it['members']) == list(range(40))      # every sequence, once
        assert c['random_state'] is not None or not c['shuffle']
    # the shuffled order differs from the given one, and truncation shortens something
    by = {(c['token_per_batch'], c['shuffle'], c['truncate_len']): c for c in g['cases']}
    b = g['cases'][0]['token_per_batch']
    assert [it['members'] for it in by[(b, True, None)]['items']] != [it['members'] for it in by[(b, False, None)]['items']]
    assert sum(len(it['token']) for it in by[(b, False, 16)]['items']) < sum(len(it['token']) for it in by[(b, False, None)]['items'])


@pytest.mark.parametrize('n', range(8), ids=_ids())
def test_labeled_dataset_yields_what_the_reference_yields(n):
    g = _golden()
    c = g['cases'][n]
    ds = LabeledDataset(g['seqs'], g['labels'], c['token_per_batch'], shuffle=c['shuffle'], random_state=c['random_state'],
                        truncate_len=c['truncate_len'])
    assert len(ds) == len(c['items'])
    for i, want in enumerate(c['items']):
        assert list(ds.sampler[i]) == want['members'], i                     # batch membership, in order
        it = ds[i]
        assert set(it) == {'token', 'cu_lens', 'max_len', 'indices', 'label'}
        assert it['token'].tolist() == want['token'] and it['cu_lens'].tolist() == want['cu_lens'], i
        assert int(it['max_len']) == want['max_len'] and it['indices'].tolist() == want['indices'], i
        assert it['label'].dtype == torch.float32 and it['label'].tolist() == want['label'], i
        assert it['token'].ndim == 1 and it['cu_lens'][-1] == it['token'].numel()


def test_labeled_dataset_details():
    seqs, labels = ['ACD', 'WWWWWW', 'K'], [1, 2.5, -3]
    ds = LabeledDataset(seqs, labels, token_per_batch=100, shuffle=False, truncate_len=4)
    assert [list(b) for b in ds.sampler] == [list(b) for b in TokenSizeBatchSampler([3, 6, 1], 100, shuffle=False)] == [[0, 1, 2]]
    it = ds[0]
    assert it['cu_lens'].tolist() == [0, 5, 11, 14] and it['max_len'] == 6 and it['label'].tolist() == [1.0, 2.5, -3.0]
    assert ds.truncate('WWWWWW') == 'WWWW' and ds.truncate('K') == 'K'
    batches = list(ds.to_dataloader())
    assert len(batches) == 1 and torch.equal(batches[0]['token'], it['token']) and torch.equal(batches[0]['label'], it['label'])
    with pytest.raises(ValueError, match='2 labels'):
        LabeledDataset(seqs, labels[:2], 100)


# ------------------------------------------------------------------ forward_trainable(layers=...)

def _model(tmp_path, kind='esm2'):
    path = syn.write_checkpoint(str(tmp_path / f'{kind}.safetensors'), f'{kind}_t', 3, 64, 2, seed=5)
    return ESM.from_pretrained(path, device='cpu')


TOK, PAD = torch.zeros(4, dtype=torch.long), (torch.tensor([0, 4], dtype=torch.int32), 4)


@pytest.mark.parametrize('kind', ('esm2', 'esmc'))
def test_layer_taps_argument_checks_need_no_device(tmp_path, kind):
    model = _model(tmp_path, kind)
    with pytest.raises(ValueError, match='logits=False'):
        model.forward_trainable(TOK, PAD, layers=[0], logits=True)
    with pytest.raises(ValueError, match='logits=False'):
        model.forward_trainable(TOK, PAD, layers=[0])                      # (logits=True is the default)
    for call in (model.forward_trainable, model.forward_representation):   # an index out of range fails as forward_representation's does
        with pytest.raises(AssertionError, match='Invalid layer indices'):
            call(TOK, PAD, layers=[3], **({'logits': False} if call == model.forward_trainable else {}))
    # without taps the call goes on to the kernels (and finds no device): the new argument's checks come after the old refusals
    for layers in (None, []):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            model.forward_trainable(TOK, PAD, logits=False, layers=layers)
    model.set_precision('high')
    with pytest.raises(NotImplementedError, match="precision 'high' has no backward"):
        model.forward_trainable(TOK, PAD, layers=[7], logits=True)         # an existing refusal is evaluated before the new argument


# ------------------------------------------------------------------ esme.trainer

def test_regression_model_host_side(tmp_path):
    from esme.pooling import BinaryLearnedAggregation
    from esme.trainer import RegressionModel
    model = _model(tmp_path)
    for p in model.parameters():
        p.requires_grad_(False)
    head = BinaryLearnedAggregation(2, 64 * 3).requires_grad_(True)
    net = RegressionModel(model, head, layers=[0, 2])
    assert net.width == 192 and net.layers == [0, 2] and not net.backbone_trains()
    assert isinstance(net, torch.nn.Module) and {n.split('.')[0] for n, _ in net.named_parameters()} == {'plm', 'head'}
    groups = net.param_groups(lr=1e-5, lr_head=1e-4)
    assert len(groups) == 1 and groups[0]['lr'] == 1e-4 and len(groups[0]['params']) == len(list(head.parameters()))
    model.mark_trainable(layers=[-1])
    groups = net.param_groups(lr=1e-5, lr_head=1e-4)
    assert [g['lr'] for g in groups] == [1e-4, 1e-5] and net.backbone_trains()
    assert len(groups[1]['params']) == len([p for p in model.parameters() if p.requires_grad]) > 0
    import esme
    opt = esme.optim.AdamW(groups)                                         # (construction needs no device)
    assert [g['lr'] for g in opt.param_groups] == [1e-4, 1e-5]
    with pytest.raises(AssertionError, match='Invalid layer indices'):
        RegressionModel(model, head, layers=[3])
    with pytest.raises(ValueError, match='Unknown reduction'):
        RegressionModel(model, head, reduction='max')
    x = torch.arange(24, dtype=torch.float32).view(2, 3, 4)
    assert torch.equal(RegressionModel(model, head, reduction='mean').reduce(x), x.mean(dim=1))
    assert torch.equal(RegressionModel(model, head, reduction='sum').reduce(x), x.sum(dim=1))
    with pytest.raises(ValueError, match='pad_output=True'):
        RegressionModel(model, head, reduction='sum').reduce(x[0])


def test_spearman():
    from esme.trainer import spearman
    x = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0])
    assert spearman(x, x * 3 + 1) == pytest.approx(1.0) and spearman(x, -x.exp()) == pytest.approx(-1.0)
    # 1 - 6 sum d^2 / (n (n^2 - 1)) without ties: ranks (1 2 3 4 5) against (2 1 4 3 5): d^2 = 4
    assert spearman(x, torch.tensor([0.2, 0.1, 0.9, 0.5, 7.0])) == pytest.approx(1 - 6 * 4 / (5 * 24))
    # ties take the average rank: (1, 2.5, 2.5, 4) against (1, 2, 3, 4): Pearson of the ranks
    a, b = torch.tensor([1.0, 2.5, 2.5, 4.0]), torch.tensor([1.0, 2.0, 3.0, 4.0])
    want = float(((a - a.mean()) @ (b - b.mean())) / ((a - a.mean()).norm() * (b - b.mean()).norm()))
    assert spearman(torch.tensor([0.0, 1.0, 1.0, 2.0]), b) == pytest.approx(want)
    assert spearman(torch.ones(4), b) != spearman(torch.ones(4), b)       # a constant has no rank correlation: nan
