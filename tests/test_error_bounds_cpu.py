"""The per-element bound recipes of tests/error_bounds.py, tested on the CPU before they judge kernels.

Correct kernels are emulated in numpy / torch: fp32 accumulation of the exact bf16 products in several orders, the output
rounded to nearest even.  Every recipe must accept them (the margin is printed).  Then a list of defects, each applied to an
emulated correct output: the new recipe must reject each, and for each the test records whether the assertion the suite used
before (check() of test_hip_kernels.py, or a whole-tensor rel-Frobenius bound) accepts it -- which gap each recipe closes.
No kernel runs and nothing touches a GPU.
"""
import math

import numpy as np
import pytest
import torch

import error_bounds as eb

BF = torch.bfloat16
H16 = torch.float16


def rnd(shape, seed, scale=1.0, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def old_check_accepts(got, ref, rtol=2.0 ** -7, atol_scale=2.0 ** -7, mag=None):
    """test_hip_kernels.check() as a predicate: |got - ref| <= atol_scale rms(ref) + rtol |ref| (or rtol mag)."""
    got, ref = got.double(), ref.double()
    atol = atol_scale * float(ref.pow(2).mean().sqrt())
    return bool(((got - ref).abs() <= atol + rtol * (ref.abs() if mag is None else mag.double())).all())


def rel_fro(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def rejects(got, ref, bound):
    try:
        eb.assert_bounded(got, ref, bound, 'defect')
    except AssertionError as e:
        return str(e)
    return None


# ------------------------------------------------------------------ emulated accumulation

def _trunc32(x64):
    """float64 -> float32 rounded toward zero."""
    f = x64.astype(np.float32)
    over = np.abs(f.astype(np.float64)) > np.abs(x64)
    f[over] = np.nextafter(f[over], np.float32(0))
    return f


def accumulate(a, w, order):
    """fp32 accumulation of the exact products a[m, k] w[n, k] (bf16 x bf16 is exact in fp32)."""
    a32, w32 = a.float().numpy(), w.float().numpy()
    M, K = a32.shape
    N = w32.shape[0]
    if order == 'sequential':
        acc = np.zeros((M, N), np.float32)
        for k in range(K):
            acc = acc + np.outer(a32[:, k], w32[:, k]).astype(np.float32)
        return acc
    if order in ('pairwise', 'blocked64'):
        parts = []
        for k0 in range(0, K, 64):
            p = a32[:, None, k0:k0 + 64] * w32[None, :, k0:k0 + 64]      # exact in fp32
            if order == 'pairwise':
                while p.shape[-1] > 1:
                    p = (p[..., 0::2] + p[..., 1::2]).astype(np.float32)
                parts.append(p[..., 0])
            else:
                s = np.zeros((M, N), np.float32)
                for j in range(p.shape[-1]):
                    s = s + p[..., j]
                parts.append(s)
        if order == 'blocked64':
            acc = np.zeros((M, N), np.float32)
            for s in parts:
                acc = acc + s
            return acc
        while len(parts) > 1:
            nxt = [(parts[i] + parts[i + 1]).astype(np.float32) for i in range(0, len(parts) - 1, 2)]
            if len(parts) % 2:
                nxt.append(parts[-1])
            parts = nxt
        return parts[0]
    if order == 'mfma32_trunc':      # 32 products per MFMA step summed exactly, added to a truncating fp32 accumulator
        acc = np.zeros((M, N), np.float32)
        a64, w64 = a32.astype(np.float64), w32.astype(np.float64)
        for k0 in range(0, K, 32):
            acc = _trunc32(acc.astype(np.float64) + a64[:, k0:k0 + 32] @ w64[:, k0:k0 + 32].T)
        return acc
    raise ValueError(order)


ORDERS = ['sequential', 'pairwise', 'blocked64', 'mfma32_trunc']


@pytest.mark.parametrize('K,M,N', [(64, 400, 256), (640, 320, 320), (5120, 160, 128)])
@pytest.mark.parametrize('order', ORDERS)
def test_c_dot_covers_fp32_accumulation(K, M, N, order):
    """C_DOT sized by emulation: the fp32 accumulators of every order stay inside C_DOT 2^-24 sqrt(K) ||a o w||_2."""
    a, w = rnd((M, K), 1 + K), rnd((N, K), 2 + K, 1 / math.sqrt(K))
    acc = torch.from_numpy(accumulate(a, w, order))
    exact = a.double() @ w.double().T
    r = eb.assert_bounded(acc, exact, eb.dot_term(a, w), f'fp32 accumulation {order} K={K}')
    print(f'\n[C_DOT] {order:13s} K={K:5d}: worst err / bound {r:.3f}')


@pytest.mark.parametrize('order', ['sequential', 'pairwise', 'blocked64', 'mfma32_trunc'])
def test_gemm_recipes_accept_correct_kernels(order):
    """Plain, bias, GELU (degree 7 and 5 polynomials emulated by float64 GELU + the output rounding), residual and SwiGLU."""
    M, N, K = 192, 256, 640
    a, w, b = rnd((M, K), 3), rnd((N, K), 4, 1 / math.sqrt(K)), rnd((N,), 5, 0.5)
    r = rnd((M, N), 6)
    acc = torch.from_numpy(accumulate(a, w, order)).double()
    margins = {}
    y32 = (acc + b.double()).float()
    for epi in ('none', 'gelu', 'residual'):
        if epi == 'none':
            got = y32.to(BF)
        elif epi == 'gelu':
            got = eb.gelu64(y32.double()).float().to(BF)
        else:
            got = (r.float() + 0.75 * y32).to(BF)
        ref, bound, _ = eb.gemm_reference(a, w, b, epi, resid=r, alpha=0.75)
        margins[epi] = eb.assert_bounded(got, ref, bound, f'gemm {epi} {order}')
    wa, wf = w[:128], w[128:]
    g32, f32 = acc[:, :128].float(), acc[:, 128:].float()
    got = (g32 * torch.sigmoid(g32) * f32).to(BF)
    ref, bound, _ = eb.swiglu_reference(a, wa, wf)
    margins['swiglu'] = eb.assert_bounded(got, ref, bound, f'gemm swiglu {order}')
    print(f'\n[gemm recipes, {order}] ' + ', '.join(f'{k} {v:.3f}' for k, v in margins.items()))


def emulate_attention(q, k, v, cu, H, scale, p_dtype, o_dtype, bad_item=None, bad_p=None, bad_o=None):
    """fp32 scores / softmax / accumulators, P rounded to p_dtype before PV, output rounded to o_dtype.  bad_item = (seq, head,
    64-row item): that work item uses bad_p for P and / or bad_o for its output instead."""
    T, E = q.shape
    d = E // H
    out = torch.empty(T, E, dtype=torch.float32)
    cl = cu.tolist()
    for si, (s0, s1) in enumerate(zip(cl[:-1], cl[1:])):
        qq, kk, vv = (t[s0:s1].float().view(-1, H, d).transpose(0, 1) for t in (q, k, v))
        s = (qq @ kk.transpose(1, 2)) * scale
        p = torch.exp(s - s.max(-1, keepdim=True).values)
        l = p.sum(-1, keepdim=True)
        pr = p.to(p_dtype).float()
        o = (pr @ vv) / l
        o = o.to(o_dtype).float()
        if bad_item is not None and bad_item[0] == si:
            h, it = bad_item[1], bad_item[2]
            rows = slice(64 * it, 64 * (it + 1))
            pb = p.to(bad_p or p_dtype).float()
            ob = ((pb @ vv) / l).to(bad_o or o_dtype).float()
            o[h, rows] = ob[h, rows]
        out[s0:s1] = o.transpose(0, 1).reshape(-1, E)
    return out


def _cu(lengths):
    return torch.tensor(np.cumsum([0] + list(lengths)), dtype=torch.int32)


def test_attention_recipe_accepts_correct_kernels():
    lengths = [1, 2, 63, 64, 65, 128, 129, 300]
    H, d = 4, 64
    T, E = sum(lengths), H * d
    cu = _cu(lengths)
    margins = {}
    for name, dt, pf in (('bf16', BF, 'bf16'), ('fp16', H16, 'fp16')):
        q, k, v = (rnd((T, E), 10 + i, dtype=dt) for i in range(3))
        got = emulate_attention(q, k, v, cu, H, d ** -0.5, dt, dt)
        ref, bound, pre = eb.attention_reference(q, k, v, cu, H, d ** -0.5, pf, pf)
        margins[name] = eb.assert_bounded(got, ref, bound, f'attention {name}', eb.attn_layout(cu, H, d))
    print('\n[attention recipe] ' + ', '.join(f'{k} {v:.3f}' for k, v in margins.items()))


def test_row_recipes_accept_correct_kernels():
    x = (rnd((300, 640), 20, 2.0).float() + 0.5).to(BF)
    w, b = (1 + 0.1 * rnd((640,), 21).float()).to(BF), rnd((640,), 22, 0.1)
    x32 = x.float()
    mean = x32.mean(1, keepdim=True)
    xc = x32 - mean
    rstd = torch.rsqrt((xc * xc).mean(1, keepdim=True) + 1e-5)
    got = (xc * rstd * w.float() + b.float()).to(BF)
    ref, bound, _ = eb.layernorm_reference(x, w, b, 1e-5, 'bf16')
    m1 = eb.assert_bounded(got, ref, bound, 'layernorm')
    lg = rnd((500, 33), 23, 3.0).float()
    m2 = eb.assert_bounded(torch.log_softmax(lg, 1).to(BF), *eb.softmax_reference(lg, True, 'bf16')[:2], 'log_softmax')
    m3 = eb.assert_bounded(torch.softmax(lg, 1), *eb.softmax_reference(lg, False, 'fp32')[:2], 'softmax fp32')
    print(f'\n[row recipes] layernorm {m1:.3f}, log_softmax {m2:.3f}, softmax fp32 {m3:.3f}')


def _f32(x):
    return x.float().double()


@pytest.mark.parametrize('kind', ['plain', 'dc20', 'outlier'])
def test_ln_fold_recipe_accepts_the_kernels_fp32_arithmetic(kind):
    """gemm.hip:333-337 and :582 (gemm_bf16_kernel: the LN-fold row statistics and its epilogue fma) emulated step by step in fp32 (fma as the float64 value of the exact product-sum, rounded once)."""
    T, E, N = 300, 640, 256
    g = torch.Generator().manual_seed(len(kind))
    x = torch.randn(T, E, generator=g) * 1.5
    if kind == 'dc20':
        x = x + 20.0
    elif kind == 'outlier':
        x[:, 7] *= 60.0
    x = x.to(BF)
    wp = (torch.randn(N, E, generator=g) * E ** -0.5).to(BF)
    c1 = wp.double().sum(1).float()
    c2 = (0.1 * torch.randn(N, generator=g)).float()
    xd = x.double()
    sums = torch.stack((xd.sum(1), (xd * xd).sum(1)), 1).float()      # fp32 partials as handed to the kernel
    inv = _f32(torch.tensor(1.0 / E))
    mean = _f32(sums[:, :1].double() * inv)
    var = _f32(_f32(sums[:, 1:].double() * inv) - _f32(mean * mean)).clamp(min=0)
    rstd = _f32(1.0 / torch.sqrt(_f32(var + 1e-5)))
    rm = _f32(rstd * mean)
    acc = torch.from_numpy(accumulate(x, wp, 'blocked64')).double()
    y = _f32(rstd * acc + _f32(-rm * c1.double() + c2.double()))
    ref, pre = eb.ln_fold_reference(x, wp, c1, c2, 1e-5, sums)
    r = eb.assert_bounded(y.float().to(BF), ref, pre + eb.out_round(ref, pre, 'bf16'), f'LN fold {kind}')
    r0 = eb.assert_bounded(y, ref, pre, f'LN fold {kind} before the output rounding')
    print(f'\n[LN fold {kind}] worst err / bound {r:.3f} (before the output rounding {r0:.3f})')


def test_rotary_recipe_accepts_fp32_rotation():
    from oracle import esm_oracle as O
    lengths, H, d = [60, 40, 180], 4, 32
    T, E = sum(lengths), H * d
    x = rnd((T, E), 41)
    cos, sin = O.rotary_tables(max(lengths), d, BF)
    pos = O.culen_positions(_cu(lengths))
    got = O.apply_rotary(x.float().view(T, H, d), cos.float(), sin.float(), pos).view(T, E).to(BF)
    ref, bnd = eb.rotary_bound(x.double().view(T, H, d), torch.zeros(T, H, d, dtype=torch.float64), cos, sin, pos)
    ref, bnd = ref.view(T, E), bnd.view(T, E)
    print(f'\n[rotary] worst err / bound {eb.assert_bounded(got, ref, bnd + eb.out_round(ref, bnd, "bf16"), "rotary"):.3f}')


def test_ulp_and_pair_resolution():
    x = torch.tensor([1.0, 1.5, 2.0, 0.0, 2.0 ** -130, 65504.0, 2.0 ** -20], dtype=torch.float64)
    assert eb.ulp(x, 'bf16').tolist()[:4] == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -133]
    assert float(eb.ulp(x, 'bf16')[4]) == 2.0 ** -133                 # subnormal floor
    assert float(eb.ulp(x, 'fp16')[5]) == 32.0 and float(eb.ulp(x, 'fp16')[6]) == 2.0 ** -24
    assert float(eb.ulp(x, 'fp32')[0]) == 2.0 ** -23
    # a (hi, lo) bf16 pair of 1.x resolves 2^-16 (lo <= 2^-8 carries 8 bits)
    assert float(eb.pair_resolution(x[:1], 'bf16')[0]) == 2.0 ** -15
    # and the pair split of random fp32 values is within half of it
    v = torch.randn(10000, dtype=torch.float64).float()
    hi = v.to(BF)
    lo = (v - hi.float()).to(BF)
    err = (hi.double() + lo.double() - v.double()).abs()
    assert bool((err <= 0.5 * eb.pair_resolution(v, 'bf16')).all())


def test_rounding_bias_tells_nearest_from_truncation():
    y = torch.randn(200000, dtype=torch.float64) * 3
    pre = torch.zeros_like(y)
    near = y.float().to(BF)
    b0, n = eb.rounding_bias(near, y, pre, 'bf16')
    trunc = _trunc_bf16(y.float())
    b1, _ = eb.rounding_bias(trunc, y, pre, 'bf16')
    print(f'\n[rounding bias] nearest {b0:+.4f}, truncation {b1:+.4f} (n = {n})')
    assert n >= 10 ** 5 and abs(b0) < 0.05 and b1 < -0.4


def _trunc_bf16(x32):
    """fp32 -> bf16 by dropping the low 16 bits (truncation toward zero)."""
    bits = x32.contiguous().view(torch.int32) & ~0xFFFF
    return bits.view(torch.float32).to(BF)


# ------------------------------------------------------------------ defects

def test_defect_gemm_output_truncated():
    M, N, K = 1000, 1280, 640
    a, w, b = rnd((M, K), 30), rnd((N, K), 31, 1 / math.sqrt(K)), rnd((N,), 32, 0.1)
    y32 = (a.float() @ w.float().T + b.float())
    got = _trunc_bf16(y32)
    ref, bound, pre = eb.gemm_reference(a, w, b)
    assert old_check_accepts(got, ref), 'check() was expected to accept a truncating GEMM'
    assert rejects(got, ref, bound)
    bias, n = eb.rounding_bias(got, ref, pre, 'bf16')
    assert n >= 10 ** 5 and bias < -0.4, (bias, n)
    print(f'\n[defect truncation] check() accepts; recipe rejects; bias {bias:+.3f} over {n}')


def test_defect_bias_added_after_output_rounding():
    M, N, K = 512, 512, 640
    a, w = rnd((M, K), 33), rnd((N, K), 34, 1 / math.sqrt(K))
    b = rnd((N,), 35, 1.0)
    acc = a.float() @ w.float().T
    got = (acc.to(BF).float() + b.float()).to(BF)                   # two roundings
    ref, bound, _ = eb.gemm_reference(a, w, b)
    assert old_check_accepts(got, ref)
    assert rejects(got, ref, bound)


def test_defect_k_tile_missing_in_last_row_tile():
    M, N, K = 1000, 256, 5120
    a, w = rnd((M, K), 36), rnd((N, K), 37, 1 / math.sqrt(K))
    acc = a.float() @ w.float().T
    last = (M // 128) * 128
    acc[last:] -= a[last:, K - 64:].float() @ w[:, K - 64:].float().T
    got = acc.to(BF)
    ref, bound, _ = eb.gemm_reference(a, w)
    msg = rejects(got, ref, bound)
    assert msg and 'row tile 7' in (lambda: _where_msg(got, ref, bound))()
    print(f'\n[defect missing K-tile] check() accepts: {old_check_accepts(got, ref)}')


def _where_msg(got, ref, bound):
    try:
        eb.assert_bounded(got, ref, bound, 'k-tile', eb.gemm_layout())
    except AssertionError as e:
        return str(e)
    return ''


def test_defect_rotary_position_off_by_one_on_last_row():
    from oracle import esm_oracle as O
    lengths, H, d = [60, 40, 180], 4, 32
    T, E = sum(lengths), H * d
    cu = _cu(lengths)
    x = rnd((T, E), 40)
    cos, sin = O.rotary_tables(max(lengths) + 1, d, BF)
    pos = O.culen_positions(cu)
    bad = pos.clone()
    bad[int(cu[2]) - 1] += 1                                          # sequence 1's last row
    got = O.apply_rotary(x.float().view(T, H, d), cos.float(), sin.float(), bad).view(T, E).to(BF)
    ref, bnd = eb.rotary_bound(x.double().view(T, H, d), torch.zeros(T, H, d, dtype=torch.float64), cos, sin, pos)
    ref, bnd = ref.view(T, E), bnd.view(T, E)
    bnd = bnd + eb.out_round(ref, bnd, 'bf16')
    assert rejects(got, ref, bnd)
    print(f'\n[defect rotary position] check() accepts: {old_check_accepts(got, ref)}')


ATTN_LENGTHS = [5, 64, 333, 1, 130, 700]


def _half_attention_case():
    H, d = 8, 64
    T, E = sum(ATTN_LENGTHS), H * d
    g = torch.Generator().manual_seed(7 * d)
    x = torch.randn(T, 3 * E, generator=g).to(H16)
    cu = _cu(ATTN_LENGTHS)
    q, k, v = x[:, :E], x[:, E:2 * E], x[:, 2 * E:]
    ref, bound, pre = eb.attention_reference(q, k, v, cu, H, d ** -0.5, 'fp16', 'fp16')
    return q, k, v, cu, H, d, ref, bound


@pytest.mark.parametrize('defect', ['bf16 P and output', 'bf16 output'])
def test_defect_half_attention_one_work_item_at_bf16(defect):
    q, k, v, cu, H, d, ref, bound = _half_attention_case()
    good = emulate_attention(q, k, v, cu, H, d ** -0.5, H16, H16)
    bad_p = BF if defect == 'bf16 P and output' else None
    bad = emulate_attention(q, k, v, cu, H, d ** -0.5, H16, H16, bad_item=(5, 3, 4), bad_p=bad_p, bad_o=BF)
    eb.assert_bounded(good, ref, bound, 'correct fp16 attention')
    assert rel_fro(good, ref) <= 6e-4 and rel_fro(bad, ref) <= 6e-4, (rel_fro(good, ref), rel_fro(bad, ref))
    msg = rejects(bad, ref, bound)
    assert msg
    try:
        eb.assert_bounded(bad, ref, bound, 'attention', eb.attn_layout(cu, H, d))
    except AssertionError as e:
        assert 'sequence 5' in str(e) and 'head 3' in str(e) and 'work item 4' in str(e), str(e)
    print(f'\n[defect half attention, {defect}] rel-Frobenius {rel_fro(bad, ref):.2e} (correct {rel_fro(good, ref):.2e}) accepted by '
          f'<= 6e-4; recipe rejects')


@pytest.mark.parametrize('p_fmt,p_dtype', [('bf16', BF), ('fp16', H16)])
def test_c_dot_covers_p_rounding(p_fmt, p_dtype):
    """The P-rounding term u_P (C_DOT ||p o v||_2 + |o|) of attention_reference, sized directly: the numerator error sum_j (fl(p_j) - p_j) v_j / l
    of rows of 2 to 1253 keys, score spreads of 0.5 to 8 log2 units against a reference that is not the row maximum (the speculative /
    deferred forms, up to the defer-max threshold 2^8), v of either sign or all positive, and rows whose keys all tie (spread 0: every P
    rounds alike, the |o| part)."""
    g = torch.Generator().manual_seed(17)
    u = eb.P_UNIT[p_fmt]
    worst = {}
    for L in (2, 64, 700, 1253):
        for spread in (0.0, 0.5, 2.0, 8.0):
            for signed in (True, False):
                t = torch.randn(64, L, generator=g, dtype=torch.float64) * spread - 3.0 * torch.rand(64, 1, generator=g, dtype=torch.float64)
                t = t.clamp(max=8.0)                                  # P <= 2^8: the defer-max threshold (larger P: the overflow redo)
                p = torch.exp2(t).float().double()                      # the fp32 P the kernel rounds
                v = torch.randn(L, 64, generator=g).to(p_dtype).double()
                if not signed:
                    v = v.abs()
                l = p.sum(-1, keepdim=True)
                err = ((p.to(p_dtype).double() - p) @ v / l).abs()
                pn = p / l
                bound = u * (eb.C_DOT * torch.sqrt((pn * pn) @ (v * v)) + (pn @ v).abs())
                if p_fmt == 'fp16':                                   # P in fp16's subnormals: the recipe's separate floor term
                    bound = bound + 2.0 ** -25 * v.abs().sum(0, keepdim=True) / l
                key = f'L={L} spread={spread}{"" if signed else " v>0"}'
                worst[key] = eb.assert_bounded(err, torch.zeros_like(err), bound, f'P rounding {p_fmt} {key}')
    print(f'\n[C_DOT, P rounding {p_fmt}] worst ' + ', '.join(f'{k}: {r:.2f}' for k, r in sorted(worst.items(), key=lambda kv: -kv[1])[:4]))


def emulate_fixed_reference(qs, k, v, cu, H, redo=True, item_rows=eb.FIXED_REF_ITEM_ROWS):
    """The fixed-reference fp16 form: t = qs . k in fp32 (log2 units), P = fp16(2^(t - 4)), l the fp32 sum of the unrounded P; a work item with a
    row whose l falls below S * 2^-14 is redone with P = fp16(2^(t - row max)) (attn.hip:1069-1076, attn_pp64_kernel).  redo = False: the defect, no redo."""
    T, E = qs.shape
    d = E // H
    out = torch.empty(T, E, dtype=torch.float32)
    cl = cu.tolist()
    for s0, s1 in zip(cl[:-1], cl[1:]):
        qq, kk, vv = (t_[s0:s1].float().view(-1, H, d).transpose(0, 1) for t_ in (qs, k, v))
        t = qq @ kk.transpose(1, 2)
        ref = torch.full_like(t[..., :1], 4.0)
        if redo:
            vanished = torch.exp2(t - 4.0).sum(-1) < (s1 - s0) * 2.0 ** -14
            for i0 in range(0, s1 - s0, item_rows):
                item = vanished[:, i0:i0 + item_rows].any(-1)
                ref[item, i0:i0 + item_rows] = t[item, i0:i0 + item_rows].amax(-1, keepdim=True)
        p = torch.exp2(t - ref)
        o = (p.to(H16).float() @ vv) / p.sum(-1, keepdim=True)
        out[s0:s1] = o.to(H16).float().transpose(0, 1).reshape(-1, E)
    return out


def _vanished_batch():
    """tests/test_attn_qp16_gpu.py's vanished-sum batch: a score offset of about -12 natural units on every key."""
    H, d, lengths = 4, 64, [300, 77, 513, 1, 65]
    T, E = sum(lengths), H * d
    g = torch.Generator().manual_seed(5)
    q, k = torch.randn(T, E, generator=g), torch.randn(T, E, generator=g)
    k[:, ::d] = 4.0
    q[:, ::d] = -12.0 / 4.0 * math.sqrt(d)
    v = torch.randn(T, E, generator=g).to(H16)
    qs = (q.to(H16).float() * (d ** -0.5 * 1.4426950408889634)).to(H16)
    return qs, k.to(H16), v, _cu(lengths), H, d


def test_defect_fixed_reference_vanished_item_not_redone():
    qs, k, v, cu, H, d = _vanished_batch()
    ref, bound, _ = eb.attention_reference(qs, k, v, cu, H, 1.0, 'fp16', 'fp16', log2_units=True, fixed_ref=4.0)
    good = emulate_fixed_reference(qs, k, v, cu, H)
    r = eb.assert_bounded(good, ref, bound, 'fixed reference, vanished items redone', eb.attn_layout(cu, H, d, eb.FIXED_REF_ITEM_ROWS))
    bad = emulate_fixed_reference(qs, k, v, cu, H, redo=False)
    assert rejects(bad, ref, bound)
    assert rejects(torch.zeros_like(good), ref, bound)
    # and a benign batch (nothing vanishes, reference 4 kept) is accepted as well
    g = torch.Generator().manual_seed(6)
    qb = (torch.randn(qs.shape, generator=g) * (d ** -0.5 * 1.4426950408889634)).to(H16)
    refb, boundb, _ = eb.attention_reference(qb, k, v, cu, H, 1.0, 'fp16', 'fp16', log2_units=True, fixed_ref=4.0)
    rb = eb.assert_bounded(emulate_fixed_reference(qb, k, v, cu, H), refb, boundb, 'fixed reference, benign')
    print(f'\n[defect vanished item not redone] correct {r:.3f}, benign {rb:.3f}; rel-Frobenius of the unredone output {rel_fro(bad, ref):.2e} '
          f'(<= 1e-3 accepts: {rel_fro(bad, ref) <= 1e-3}); recipe rejects it and an all-zero output')


def _split(x):
    hi = x.to(BF)
    return hi, (x - hi.float()).to(BF)


def test_defect_exact_pair_output_row_loses_lo():
    M, N, K = 45000, 512, 256
    g = torch.Generator().manual_seed(M + N)
    x = torch.randn(M, K, generator=g) * 3.0
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(BF)
    b = torch.randn(N, generator=g).to(BF)
    xh, xl = _split(x)
    a = torch.cat((xh, xl), 1)
    w2 = torch.cat((w, w), 1)
    ref, bound, _ = eb.gemm_reference(a, w2, b, pair=True)
    y32 = (ref + (torch.rand(ref.shape, generator=g, dtype=torch.float64) - 0.5) * eb.dot_term(a, w2)).float()   # an fp32 accumulator
    hi, lo = _split(y32)
    got = hi.double() + lo.double()
    eb.assert_bounded(got, ref, bound, 'correct pair output')
    bad = got.clone()
    bad[31337] = hi[31337].double()                                  # one row without its lo half
    assert rel_fro(bad, ref) <= 2e-5, rel_fro(bad, ref)
    assert rejects(bad, ref, bound)
    print(f'\n[defect pair row] rel-Frobenius {rel_fro(bad, ref):.2e} accepted by <= 2e-5; recipe rejects')


def test_defect_split_attention_p_rounded_to_bf16_in_one_work_item():
    lengths, H, d = [1, 7, 64, 65, 130, 300, 517], 4, 64
    T, E = sum(lengths), H * d
    cu = _cu(lengths)
    g = torch.Generator().manual_seed(d)
    qkv = torch.randn(T, 3 * E, generator=g) * 1.5
    hi, lo = _split(qkv)
    x = hi.double() + lo.double()
    q, k, v = x[:, :E], x[:, E:2 * E], x[:, 2 * E:]
    ref, bound, pre = eb.attention_reference(q, k, v, cu, H, d ** -0.5, 'bf16pair', 'bf16', pair_out=True, qk_drop=2.0 ** -16)
    # correct: fp32 softmax, P as a pair (about fp32), output as a pair
    good = emulate_attention(q.float(), k.float(), v.float(), cu, H, d ** -0.5, torch.float32, torch.float32).double()
    bad = emulate_attention(q.float(), k.float(), v.float(), cu, H, d ** -0.5, torch.float32, torch.float32,
                            bad_item=(3, 1, 1), bad_p=BF).double()      # the 65-key sequence's one-row tail item
    eb.assert_bounded(good, ref, bound, 'correct split attention')
    assert rel_fro(bad, ref) <= 2e-5, rel_fro(bad, ref)
    assert rejects(bad, ref, bound)
    print(f'\n[defect split attention bf16 P] rel-Frobenius {rel_fro(bad, ref):.2e} accepted by <= 2e-5; recipe rejects')


def test_defect_extension_tile_lo_dropped():
    """Precision 'half' with a massive stream channel: the LayerNorm-folded GEMM reads [hi | ext], ext = lo of the selected columns.
    Dropping ext leaves the massive channels at one fp16 rounding."""
    M, E, N = 512, 256, 384
    g = torch.Generator().manual_seed(3)
    x32 = torch.randn(M, E, generator=g)
    sel = torch.tensor([5, 77, 200])
    x32[:, sel] *= 300.0
    hi = x32.to(H16)
    lo = (x32 - hi.float()).to(H16)
    w = (torch.randn(N, E, generator=g) / math.sqrt(E)).to(H16)
    xs = hi.double()
    xs[:, sel] += lo[:, sel].double()                               # the operand as the kernel is handed it: hi + ext
    c1 = w.double().sum(1).float()
    c2 = (0.1 * torch.randn(N, generator=g)).float()
    ref, pre = eb.ln_fold_reference(xs, w, c1, c2, 1e-5)
    bound = pre + eb.out_round(ref, pre, 'fp16')
    good = ref.float().to(H16)
    eb.assert_bounded(good, ref, bound, 'correct LN fold with the extension tile')
    xd = hi.double()                                                 # ext dropped
    bad, _ = eb.ln_fold_reference(xd, w, c1, c2, 1e-5)
    bad = bad.float().to(H16)
    # test_half_robust_gpu judges the layer outputs by rel-Frobenius 1e-3 against the fp32 oracle
    assert rel_fro(bad, ref) <= 1e-3, rel_fro(bad, ref)
    assert rejects(bad, ref, bound)
    print(f'\n[defect ext lo dropped] rel-Frobenius {rel_fro(bad, ref):.2e} accepted by <= 1e-3; recipe rejects')
