"""The linear-chain CRF kernels (csrc/crf.hip) on the device against the float64 restatement and the per-element bound of
tests/crf_bounds.py, on its cases: eleven sequences of 0 .. 257 residues framed by SKIP rows, SKIP rows inside, free and constrained
rows, C in {1, 2, 3, 9, 33, 64}, per-sequence upstream gradients that all differ; emissions up to 80; a nearly forbidden label; operands
on the 2^-4 grid with deliberate ties, where the decoded path must EQUAL the reference's.

 - log Z, d_emissions, d_transitions, d_start, d_end and the marginals inside the bound (the worst error / bound of each is printed;
   profiles/crf_parity.txt keeps a run's output), under torch.cuda.set_sync_debug_mode('error');
 - reruns bit-equal; every sequence alone bit-equal to its slice of the packed batch; empty chains give 0;
 - esme.crf.CRF.loss and its backward against float64 autograd of a differentiable torch implementation, all three reductions;
 - NaN and +inf emissions stay in their sequence; 70 000 sequences; a strided emissions view past 2^31 elements;
 - a two-layer model with LoRA and a ResidueCRFHead trains, and predict keeps to the allowed transitions."""
import importlib.util
import os

import pytest
import torch

import crf_bounds as CB
from test_lora_gpu import tiny

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ('e', 'A', 'start', 'end', 'cu', 'tags', 'g')
_SHARED = {}


def _case(case):
    """Operands (CPU and device), the float64 reference and its bound: computed once per case, shared, never modified."""
    if case['name'] not in _SHARED:
        ops = CB.make_case(case)
        args = [ops[k] for k in ARGS]
        _SHARED[case['name']] = dict(ops=ops, dev={k: v.to(DEV) for k, v in ops.items()}, ref=CB.reference(*args, with_bound=True))
    return _SHARED[case['name']]


def _run(d, g=None, params=True):
    """Every output of the three entry points on the device operands `d`."""
    from esme import _hip_crf as HC
    ops = (d['e'], d['A'], d['start'], d['end'], d['cu'], d['tags'])
    logz, alpha = HC.crf_fwd(*ops)
    de, dA, ds, dn = HC.crf_bwd(*ops, alpha, logz, d['g'] if g is None else g, want_params=params)
    path, score = HC.crf_decode(*ops)
    return dict(logz=logz, alpha=alpha, de=de, dA=dA, dstart=ds, dend=dn, path=path, score=score)


def _strict(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        return fn()
    finally:
        torch.cuda.set_sync_debug_mode('default')


@pytest.mark.parametrize('case', CB.CASES, ids=[c['name'] for c in CB.CASES])
def test_outputs_within_the_bound(case):
    c = _case(case)
    d, ref, C = c['dev'], c['ref'], case['C']
    got = _strict(lambda: _run(d))
    worst = CB.worst_of(got, ref, case['kind'] == 'grid')
    ones = torch.ones_like(d['g'])
    marg = _strict(lambda: _run(d, ones, params=False))['de']
    cu, gcpu = c['ops']['cu'], c['ops']['g'].double()
    seq = torch.repeat_interleave(torch.arange(cu.numel() - 1), (cu[1:] - cu[:-1]).long())
    worst['marginals'] = CB.worst(marg, ref['de'] / gcpu[seq].unsqueeze(1), ref['bound']['de'] / gcpu[seq].abs().unsqueeze(1))
    print(f"\n[crf] {case['name']}: worst err / bound " + ' '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    assert bool(torch.isfinite(got['logz']).all()) and bool(torch.isfinite(got['de']).all())
    # the rows of the marginals are distributions on chain rows and zero elsewhere; alpha is zero outside chains
    tags = c['ops']['tags']
    chain = (tags >= -1) & (tags < C)
    rows, slack = marg.cpu().double().sum(1), (ref['bound']['de'] / gcpu[seq].abs().unsqueeze(1)).sum(1) + C * 2.0 ** -24
    assert bool(((rows - 1).abs() <= slack)[chain].all()) and not bool(marg.cpu()[~chain].any()) and not bool(got['alpha'].cpu()[~chain].any())
    # constrained rows decode to their label, rows outside chains to the fill
    path = got['path'].cpu()
    con = chain & (tags >= 0)
    assert torch.equal(path[con], tags[con].long()) and bool((path[~chain] == -100).all()) and bool(((path[chain] >= 0) & (path[chain] < C)).all())
    # empty chains: sequence 0 has no row, sequence 9 only its frame
    for b in (0, 9):
        assert float(got['logz'][b]) == 0.0 and float(got['score'][b]) == 0.0
    again = _run(d)
    for k in ('logz', 'alpha', 'de', 'dA', 'dstart', 'dend', 'path', 'score'):
        assert torch.equal(got[k], again[k]), f'{k} differs between two runs'
    from esme import _hip_crf as HC
    p32 = _strict(lambda: HC.crf_decode(d['e'], d['A'], d['start'], d['end'], d['cu'], d['tags'], fill=-7, dtype=torch.int32)[0])
    assert p32.dtype == torch.int32 and torch.equal(torch.where(p32 == -7, -100, p32).long(), got['path'])


@pytest.mark.parametrize('name', ['C3-free', 'C64-mixed', 'C9-grid-free', 'C33-grid'])
def test_each_sequence_alone_equals_its_slice(name):
    c = _case(next(k for k in CB.CASES if k['name'] == name))
    d = c['dev']
    full = _strict(lambda: _run(d))
    cu = c['ops']['cu'].tolist()
    for b, (a, z) in enumerate(zip(cu[:-1], cu[1:])):
        one = dict(d, e=d['e'][a:z], tags=d['tags'][a:z].clone(), cu=torch.tensor([0, z - a], dtype=torch.int32, device=DEV), g=d['g'][b:b + 1].clone())
        if (a * d['e'].shape[1]) % 4:
            one['e'] = one['e'].clone()                                               # (a 16-byte aligned base)
        got = _strict(lambda: _run(one, params=False))
        assert torch.equal(got['logz'], full['logz'][b:b + 1]) and torch.equal(got['score'], full['score'][b:b + 1]), b
        assert torch.equal(got['de'], full['de'][a:z]) and torch.equal(got['path'], full['path'][a:z]), b


# ------------------------------------------------------------------ esme.crf.CRF.loss against float64 autograd

def _logz64(e, A, start, end, cu, tags):
    """log Z per sequence in differentiable float64 torch ops (one step per chain row)."""
    C, out = e.shape[1], []
    for b in range(cu.numel() - 1):
        al = None
        for t in range(int(cu[b]), int(cu[b + 1])):
            tag = int(tags[t])
            if not -1 <= tag < C:
                continue
            v = (start if al is None else torch.logsumexp(al.unsqueeze(1) + A, 0)) + e[t]
            if tag >= 0:
                v = v + torch.where(torch.arange(C) == tag, 0.0, float('-inf')).double()
            al = v
        out.append(e.new_zeros(()) if al is None else torch.logsumexp(al + end, 0))
    return torch.stack(out)


LOSS_LENGTHS = (0, 1, 5, 0, 33, 70)


@pytest.mark.parametrize('reduction', ['sum', 'mean', 'token_mean'])
def test_crf_loss_and_backward_against_float64_autograd(reduction):
    from esme.crf import CRF, default_chain
    C = 5
    o = CB.make_case(dict(name='loss', C=C, kind='random', tags='mixed'), LOSS_LENGTHS)
    cu, T = o['cu'], o['e'].shape[0]
    chain = default_chain(cu, T)
    g = torch.Generator().manual_seed(4)
    labels = torch.where(torch.rand(T, generator=g) < 0.3, torch.full((T,), -100), torch.randint(0, C, (T,), generator=g))
    labels[5], labels[6] = C, -1                                                      # out of range: free rows
    allowed = torch.rand(C, C, generator=g) > 0.2
    crf = CRF(C, allowed=allowed).to(DEV).requires_grad_(True)
    e = o['e'].to(DEV).requires_grad_(True)

    labels_d, cu_d = labels.to(DEV), cu.to(DEV)

    def run():
        loss = crf.loss(e, labels_d, cu_d, reduction=reduction)
        loss.backward()
        return loss
    loss = _strict(run)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.grad_fn is not None
    # float64: the same function in torch ops, and the restatement of crf_bounds with its bound (the two must agree)
    A64, s64, n64 = (t.detach().cpu().double() for t in crf.scores())
    params = [t.clone().requires_grad_(True) for t in (o['e'].double(), A64, s64, n64)]
    labelled = chain & (labels >= 0) & (labels < C)
    free = torch.where(chain, CB.FREE, CB.SKIP).int()
    tags = torch.where(labelled, labels.int(), free)
    nonempty = sum(1 for b in range(cu.numel() - 1) if bool(chain[int(cu[b]):int(cu[b + 1])].any()))
    den = {'sum': 1, 'mean': max(nonempty, 1), 'token_mean': max(int(labelled.sum()), 1)}[reduction]
    want = (_logz64(*params, cu, free) - _logz64(*params, cu, tags)).sum() / den
    want.backward()
    coef = torch.full((cu.numel() - 1,), 1.0 / den, dtype=torch.float64)
    rf = CB.reference(o['e'], A64, s64, n64, cu, free, coef, with_bound=True)
    rc = CB.reference(o['e'], A64, s64, n64, cu, tags, coef, with_bound=True)
    assert abs(float(want.detach()) - float(((rf['logz'] - rc['logz']) * coef.double()).sum())) < 1e-9
    e_loss = float(((rf['bound']['logz'] + rc['bound']['logz']) * coef.double()).sum()) * 1.01 + 2.0 ** -22 * abs(float(want.detach()))
    print(f'\n[crf] loss {reduction}: {float(loss.detach()):.6f} float64 {float(want.detach()):.6f} |difference| / bound {abs(float(loss.detach()) - float(want.detach())) / e_loss:.3f}')
    assert abs(float(loss.detach()) - float(want.detach())) <= e_loss
    got = dict(de=e.grad, dA=crf.transitions.grad, dstart=crf.start_transitions.grad, dend=crf.end_transitions.grad)
    for (k, v), p in zip(got.items(), params):
        ref, bnd = rf[k] - rc[k], rf['bound'][k] + rc['bound'][k] + 2.0 ** -23 * (rf[k].abs() + rc[k].abs())      # (the two gradients are added in fp32)
        assert float((p.grad - ref).abs().max()) < 1e-9, k
        w = CB.worst(v, ref, bnd)
        print(f'[crf] loss {reduction}: {k} worst err / bound {w:.3f}')
        assert w <= 1.0, k
    assert float(got['de'].abs().sum()) > 0 and float(got['dA'].abs().sum()) > 0


def test_ignore_index_inside_the_label_range_and_no_sequence():
    from esme import _hip_crf as HC
    from esme.crf import CRF
    o = CB.make_case(dict(name='ignore', C=3, kind='random', tags='free'), LOSS_LENGTHS)
    crf, e, cu = CRF(3).to(DEV), o['e'].to(DEV), o['cu'].to(DEV)
    g = torch.Generator().manual_seed(6)
    labels = torch.randint(0, 3, (e.shape[0],), generator=g).to(DEV)
    a = crf.loss(e, labels, cu, ignore_index=2)                                     # label 2 is the ignored one: those rows are free
    b = crf.loss(e, torch.where(labels == 2, -100, labels), cu)
    assert torch.equal(a, b) and not torch.equal(a, crf.loss(e, labels, cu))
    # no sequence at all (cu_lens of one element) over T > 0 rows: zeros and the fill, nothing uninitialised
    none = torch.zeros(1, dtype=torch.int32, device=DEV)
    A, s, n = (t.detach().contiguous() for t in crf.scores())
    tags = torch.full((e.shape[0],), -1, dtype=torch.int32, device=DEV)
    logz, alpha = HC.crf_fwd(e, A, s, n, none, tags)
    de, dA, ds, dn = HC.crf_bwd(e, A, s, n, none, tags, alpha, logz, logz)
    path, score = HC.crf_decode(e, A, s, n, none, tags, fill=-5)
    assert logz.numel() == score.numel() == 0 and not bool(alpha.any()) and not bool(de.any()) and bool((path == -5).all())
    assert not bool(dA.any()) and not bool(ds.any()) and not bool(dn.any())


def test_no_labelled_row_gives_zero_loss_and_zero_gradients():
    from esme.crf import CRF
    o = CB.make_case(dict(name='nolabel', C=3, kind='random', tags='free'), LOSS_LENGTHS)
    crf = CRF(3).to(DEV).requires_grad_(True)
    for reduction in ('sum', 'mean', 'token_mean'):
        e = o['e'].to(DEV).requires_grad_(True)
        crf.zero_grad(set_to_none=True)
        loss = crf.loss(e, torch.full((e.shape[0],), -100, device=DEV), o['cu'].to(DEV), reduction=reduction)
        loss.backward()
        assert float(loss.detach()) == 0.0 and not bool(e.grad.any()) and not bool(crf.transitions.grad.any()) and not bool(crf.end_transitions.grad.any())
    empty = crf.loss(torch.zeros(0, 3, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV), torch.zeros(3, dtype=torch.int32, device=DEV))
    assert float(empty) == 0.0                                                        # no row at all: a zero denominator gives 0


# ------------------------------------------------------------------ non-finite emissions

@pytest.mark.parametrize('where', ['free', 'constrained'])
@pytest.mark.parametrize('value', [float('nan'), float('inf')])
def test_a_non_finite_emission_stays_in_its_sequence(value, where):
    """where: on a free row, or on a constrained row at a label OTHER than its tag (no path runs through that entry)."""
    c = _case(next(k for k in CB.CASES if k['name'] == 'C9-mixed'))
    d, cu, tags = c['dev'], c['ops']['cu'].tolist(), c['ops']['tags']
    clean = _run(d)
    b = 7
    t = next(t for t in range(cu[b] + 20, cu[b + 1]) if (int(tags[t]) == CB.FREE if where == 'free' else 0 <= int(tags[t]) < 9))
    e = d['e'].clone()
    e[t, (int(tags[t]) + 4) % 9 if where == 'constrained' else 4] = value
    got = _run(dict(d, e=e))
    a, z = cu[b], cu[b + 1]
    chain = ((tags >= -1) & (tags < 9))[a:z]
    assert not bool(torch.isfinite(got['logz'][b])) and not bool(torch.isfinite(got['score'][b]))
    assert not bool(torch.isfinite(got['de'][a:z].cpu()[chain]).any())                # never comes out finite
    for k in ('dA', 'dstart', 'dend'):
        assert not bool(torch.isfinite(got[k]).all()), k
    keep = torch.ones(len(cu) - 1, dtype=torch.bool)
    keep[b] = False
    assert torch.equal(got['logz'].cpu()[keep], clean['logz'].cpu()[keep]) and torch.equal(got['score'].cpu()[keep], clean['score'].cpu()[keep])
    for k in ('de', 'path', 'alpha'):
        assert torch.equal(got[k][:a], clean[k][:a]) and torch.equal(got[k][z:], clean[k][z:]), k


# ------------------------------------------------------------------ sizes

def test_seventy_thousand_sequences():
    """B = 70 000 > 65 535 sequences of three free rows at C = 3: every path enumerated in float64."""
    B, C = 70_000, 3
    g = torch.Generator().manual_seed(11)
    e, A = torch.randn(3 * B, C, generator=g), torch.randn(C, C, generator=g)
    start, end = torch.randn(C, generator=g), torch.randn(C, generator=g)
    grad = 0.5 + torch.rand(B, generator=g)
    d = dict(e=e.to(DEV), A=A.to(DEV), start=start.to(DEV), end=end.to(DEV), cu=(3 * torch.arange(B + 1, dtype=torch.int32)).to(DEV),
             tags=torch.full((3 * B,), CB.FREE, dtype=torch.int32, device=DEV), g=grad.to(DEV))
    got = _strict(lambda: _run(d))
    e3, A64 = e.double().view(B, 3, C), A.double()
    sc = (start.double()[None, :, None, None] + e3[:, 0, :, None, None] + A64[None, :, :, None] + e3[:, 1, None, :, None] + A64[None, None, :, :]
          + e3[:, 2, None, None, :] + end.double()[None, None, None, :])            # (B, y1, y2, y3)
    logz = torch.logsumexp(sc.view(B, -1), 1)
    pr = torch.exp(sc - logz[:, None, None, None]) * grad.double()[:, None, None, None]
    # per element: 40 roundings of 2^-23 relative on values of magnitude <= 20 for log Z and the marginals (three steps; cf. crf_bounds),
    # and for the sums over 2 B terms in fp32 gamma(T + B) of the summed magnitudes on top
    tol = 40 * 2.0 ** -23 * 20
    assert float((got['logz'].cpu().double() - logz).abs().max()) <= tol
    de = torch.stack((pr.sum((2, 3)), pr.sum((1, 3)), pr.sum((1, 2))), 1).view(3 * B, C)
    assert float((got['de'].cpu().double() - de).abs().max()) <= tol * 2
    dA = pr.sum(3).sum(0) + pr.sum(1).sum(0)
    # the longest chain of fp32 additions behind one element: the part's ceil(B / 1024) sequences of two moves, then the 1024 parts
    lim = CB.gamma(2 * -(-B // 1024) + 1024) * 2 * float(grad.sum()) + tol * 2 * float(grad.sum())
    assert float((got['dA'].cpu().double() - dA).abs().max()) <= lim
    assert float((got['dstart'].cpu().double() - pr.sum((2, 3)).sum(0)).abs().max()) <= lim
    assert float((got['dend'].cpu().double() - pr.sum((1, 2)).sum(0)).abs().max()) <= lim
    best = sc.view(B, -1).max(1).values
    assert float((got['score'].cpu().double() - best).abs().max()) <= tol
    p = got['path'].cpu().view(B, 3)
    mine = sc[torch.arange(B), p[:, 0], p[:, 1], p[:, 2]]
    assert float((mine - best).abs().max()) <= tol                                    # the decoded path is a best path
    print(f"\n[crf] B 70000: logz err {float((got['logz'].cpu().double() - logz).abs().max()):.2e} dA err {float((got['dA'].cpu().double() - dA).abs().max()):.2e} (limit {lim:.2e})")


def test_strided_emissions_past_two_to_the_31_elements():
    """emissions as the first two columns of a (T, ld) buffer with T ld >= 2^31: the row offsets need 64-bit arithmetic."""
    T, ld, C, B = 65_544, 32_768, 2, 66
    assert T * ld >= 2 ** 31
    buf = torch.empty(T, ld, dtype=torch.float32, device=DEV)
    g = torch.Generator().manual_seed(12)
    e = torch.randn(T, C, generator=g).to(DEV)
    buf[:, :C] = e
    view = buf[:, :C]
    assert view.stride(0) == ld and (T - 1) * ld >= 2 ** 31 - ld
    cu = torch.linspace(0, T, B + 1).round().to(torch.int32)
    tags = torch.full((T,), CB.FREE, dtype=torch.int32)
    tags[cu[:-1].long()] = CB.SKIP
    tags[::7] = torch.arange(0, T, 7, dtype=torch.int32) % C                          # constrained rows
    d = dict(A=torch.randn(C, C, generator=g).to(DEV), start=torch.randn(C, generator=g).to(DEV), end=torch.randn(C, generator=g).to(DEV),
             cu=cu.to(DEV), tags=tags.to(DEV), g=(0.5 + torch.rand(B, generator=g)).to(DEV))
    strided, plain = _run(dict(d, e=view)), _run(dict(d, e=e))
    for k in ('logz', 'de', 'dA', 'dstart', 'dend', 'path', 'score'):
        assert torch.equal(strided[k], plain[k]), k
    assert bool(torch.isfinite(plain['logz']).all()) and float(plain['de'][-1].abs().sum()) > 0      # the last rows were reached


# ------------------------------------------------------------------ end to end

def _tool():
    spec = importlib.util.spec_from_file_location('residue_finetune', os.path.join(ROOT, 'tools', 'residue_finetune.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_a_crf_head_trains_end_to_end_and_predicts_allowed_paths(tmp_path):
    import esme
    from esme.data import ResidueLabeledDataset
    from esme.head import ResidueCRFHead
    from esme.trainer import ResidueModel
    T = _tool()
    model = tiny(tmp_path, 'esm2', 2, 64, 2, 3).add_lora(rank=4, alpha=4, layers=('query', 'value', 'output'))
    model.mark_only_lora_as_trainable()
    torch.manual_seed(3)
    # the segment task's rule: 0 -> 2, 1 -> 0 and 2 -> 2 never occur
    allowed = torch.tensor([[1, 1, 0], [0, 1, 1], [1, 1, 0]], dtype=torch.bool)
    head = ResidueCRFHead(64, 3, allowed=allowed).to(DEV).requires_grad_(True)
    net = ResidueModel(model.train(), head)
    opt = esme.optim.AdamW(net.param_groups(1e-3, 1e-2), weight_decay=0.0)
    seqs, labels = T.make_segment_task(16, seed=0, lo=20, hi=60)
    labels[0][3] = -1                                                                 # an unlabelled residue inside a protein: marginalised over
    data = ResidueLabeledDataset(seqs, labels, 600, shuffle=True, random_state=0)
    batches = [data[i] for i in range(len(data))]
    token, pad_args, label = T.batch_to(batches[0], DEV)
    first = net.loss_trainable(token, pad_args, label)
    assert first.dtype == torch.float32 and first.dim() == 0 and first.grad_fn is not None
    _strict(lambda: net.loss_trainable(token, pad_args, label).backward())            # the step's loss and backward leave the host alone
    net.zero_grad(set_to_none=True)
    losses = T.train_steps(net, opt, batches, DEV, 12)
    print('\n[crf] training: ' + '  '.join(f'{l:.4f}' for l in losses))
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < losses[0]
    assert any(p.grad is not None and bool(p.grad.any()) for p in head.crf.parameters())
    net.eval()
    pred = net.predict(token, pad_args)
    assert pred.dtype == torch.int64 and pred.shape == token.shape
    cu = pad_args[0].tolist()
    ok = allowed.tolist()
    for a, z in zip(cu[:-1], cu[1:]):
        p = pred[a:z].tolist()
        assert p[0] == -100 and p[-1] == -100 and all(0 <= v < 3 for v in p[1:-1])
        assert all(ok[i][j] for i, j in zip(p[1:-2], p[2:-1])), p                    # only allowed transitions
    marg = head.marginals(net.plm.forward_representation(token, pad_args), pad_args[0])
    assert marg.shape == (token.numel(), 3) and float((marg.sum(1)[label != -100] - 1).abs().max()) < 1e-3
    acc = T.accuracy(net, batches, DEV)
    print(f'[crf] accuracy after 12 steps: {acc:.4f}')
    assert 0.0 <= acc <= 1.0
