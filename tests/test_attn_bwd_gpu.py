"""esme_hip_attn_varlen_bwd on the device against the float64 reference, inside the per-element bound of tests/attn_bwd_bounds.py
(which tests/test_attn_bwd_cpu.py shows to reject the defects a review would look for on these very shapes): the tile edges and empty
sequences, both head dims, gradients as column blocks of one buffer and as separate tensors, strided o / dO; large scores (the maximum
subtraction); bit-equal reruns; a sequence alone against its slice of the packed batch; the head dims that are refused."""
import pytest
import torch

import attn_bwd_bounds as AB

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_SHARED = {}


def _case(key, lengths, H, d, seed, gain=1.0):
    """Operands on the device, the forward kernel's o (in a buffer with a row stride of its own), the float64 reference and the
    bound: computed once per key, shared, never modified."""
    if key not in _SHARED:
        from esme import _hip
        c = AB.make_operands(lengths, H, d, seed, qk_gain=gain)
        dev = {n: c[n].to(DEV) for n in ('qkv', 'cu')}
        E = H * d
        dev['do'] = torch.zeros(c['do'].shape[0], E + 8, dtype=torch.bfloat16, device=DEV)[:, :E].copy_(c['do'])
        q, k, v = (dev['qkv'][:, i * E:(i + 1) * E] for i in range(3))
        o = torch.zeros(q.shape[0], E + 16, dtype=torch.bfloat16, device=DEV)[:, 8:8 + E]
        _hip.attn_varlen(q, k, v, dev['cu'], max(lengths), H, softmax_scale=c['scale'], out=o)
        dev.update(q=q, k=k, v=v, o=o)
        o_cpu = o.cpu()
        ref = AB.reference_bwd(c['q'], c['k'], c['v'], c['do'], c['cu'], H, d, c['scale'])[:3]
        bound = AB.bwd_bound(c['q'], c['k'], c['v'], o_cpu, c['do'], c['cu'], H, d, c['scale'])
        _SHARED[key] = dict(c, dev=dev, ref=ref, bound=bound)
    return _SHARED[key]


def _run(c, layout='blocks'):
    from esme import _hip_attn_bwd as HB
    d = c['dev']
    ml = max(c['lengths'])
    if layout == 'blocks':
        return HB.attn_varlen_bwd(d['q'], d['k'], d['v'], d['o'], d['do'], d['cu'], ml, c['H'], c['scale'])
    q, k, v = (t.contiguous() for t in (d['q'], d['k'], d['v']))
    outs = tuple(torch.full_like(q, float('nan')) for _ in range(3))
    return HB.attn_varlen_bwd(q, k, v, d['o'], d['do'], d['cu'], ml, c['H'], c['scale'], *outs)


@pytest.mark.parametrize('layout', ('blocks', 'separate'))
@pytest.mark.parametrize('d', (32, 64))
def test_gradients_inside_the_bound(d, layout):
    c = _case(('edges', d), AB.LENGTHS, AB.HEADS, d, seed=3 + d)
    got = _run(c, layout)
    torch.cuda.synchronize()
    for name, g, r, b in zip(('dq', 'dk', 'dv'), got, c['ref'], c['bound']):
        ratio = float(((g.double().cpu() - r).abs() / b).max())
        print(f'd {d} {layout} {name}: worst err / bound {ratio:.3f}, largest |ref| {float(r.abs().max()):.3f}')
        assert bool(torch.isfinite(g.float()).all()), name
        assert ratio <= 1.0, f'{name}: err / bound {ratio:.2f}'
    if layout == 'blocks':
        assert got[0].stride(0) == got[1].stride(0) == got[2].stride(0) == 3 * AB.HEADS * d and got[1].data_ptr() - got[0].data_ptr() == 2 * AB.HEADS * d


def test_large_scores():
    """One 300-row sequence, H = 2, d = 64, q and k scaled until the largest |score * scale| is about 40 natural units: exp() of such a
    score without the row maximum subtracted overflows bf16 / fp32 products; the statistics pass must carry it."""
    c = _case('large', (300,), 2, 64, seed=9, gain=2.45)
    q, k = (c[n].double().reshape(300, 2, 64) for n in ('q', 'k'))
    top = float((torch.einsum('ihc,jhc->hij', q, k) * c['scale']).abs().max())
    print(f'largest |score * scale| {top:.1f}')
    assert 30.0 <= top <= 60.0
    got = _run(c)
    torch.cuda.synchronize()
    for name, g, r, b in zip(('dq', 'dk', 'dv'), got, c['ref'], c['bound']):
        ratio = float(((g.double().cpu() - r).abs() / b).max())
        print(f'large scores {name}: worst err / bound {ratio:.3f}, largest |ref| {float(r.abs().max()):.3f}')
        assert bool(torch.isfinite(g.float()).all()) and ratio <= 1.0, f'{name}: err / bound {ratio:.2f}'


@pytest.mark.parametrize('d', (32, 64))
def test_reruns_are_bit_equal_and_sequences_independent(d):
    from esme import _hip_attn_bwd as HB
    c = _case(('edges', d), AB.LENGTHS, AB.HEADS, d, seed=3 + d)
    a, b = _run(c), _run(c)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    dev, cu = c['dev'], [int(x) for x in c['cu']]
    for s, n in enumerate(c['lengths']):
        lo, hi = cu[s], cu[s + 1]
        one = torch.tensor([0, n], dtype=torch.int32, device=DEV)
        alone = HB.attn_varlen_bwd(dev['q'][lo:hi], dev['k'][lo:hi], dev['v'][lo:hi], dev['o'][lo:hi], dev['do'][lo:hi], one, max(n, 1), c['H'], c['scale'])
        for x, y in zip(alone, a):
            assert torch.equal(x, y[lo:hi]), f'sequence {s} (length {n}) differs alone and packed'


def test_empty_sequences_write_nothing():
    from esme import _hip_attn_bwd as HB
    c = AB.make_operands((0, 0), 2, 32, seed=1)
    z = torch.zeros(8, 64, dtype=torch.bfloat16, device=DEV)
    outs = tuple(torch.full_like(z, 7.0) for _ in range(3))
    HB.attn_varlen_bwd(z, z.clone(), z.clone(), z.clone(), z.clone(), c['cu'].to(DEV), 4, 2, c['scale'], *outs)
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == 7.0).all())


@pytest.mark.parametrize('d', (16, 128))
def test_other_head_dims_are_refused(d):
    from esme import _hip_attn_bwd as HB
    z = torch.zeros(4, 2 * d, dtype=torch.bfloat16, device=DEV)
    cu = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match=r'code -2.*head dim must be 32 or 64'):
        HB.attn_varlen_bwd(z, z.clone(), z.clone(), z.clone(), z.clone(), cu, 4, 2, d ** -0.5)
