"""Per-element error bounds for the HIP kernels, written as the sum of the rounding steps each kernel performs.

A kernel result is judged element by element against a float64 reference computed from the exact operands the kernel
was handed (bf16 / fp16 values, or hi + lo pairs):  |got - ref64| <= bound, with no rms floor.  Every recipe below is the
sum of the kernel's own rounding steps; each step cites the kernel line that performs it.  Nothing here is tuned to a GPU
run: the one statistical constant, C_DOT, is sized by CPU emulations (tests/test_error_bounds_cpu.py).

Units: U32 = 2^-24 is fp32's unit roundoff (half an ulp at 1.0).  All helpers take and return torch tensors and work on
any device (the GPU tests form their float64 references on the GPU to keep the run short).
"""
import math

import torch

U32 = 2.0 ** -24
# fp32 accumulation of exact bf16 / fp16 products inside the MFMA chain.  The hardware's internal order is not documented,
# so the dot-product term is statistical:  C_DOT * 2^-24 * sqrt(K) * ||a_row o w_col||_2.  C_DOT = 4 covers sequential,
# pairwise and 64-blocked fp32 accumulation with round-to-nearest at every product, and a 32-product MFMA step added to a
# TRUNCATING fp32 accumulator, over 10^5-element outputs at K up to 5120 (test_error_bounds_cpu.py::test_c_dot_covers_*
# prints the worst ratio of each).
C_DOT = 4.0
# v_exp_f32 / v_rcp_f32 / v_rsq_f32 / v_log_f32 (__builtin_amdgcn_exp2f, __builtin_amdgcn_rcpf, rsqrtf, __expf, __logf): the ISA
# states 1 ulp for these; a relative error of 2^-23 per use.
E_TRANS = 2.0 ** -23

FORMATS = {                 # significand bits (implicit bit included), smallest normal exponent
    'bf16': (8, -126),
    'fp16': (11, -14),
    'fp32': (24, -126),
}
TORCH_FMT = {torch.bfloat16: 'bf16', torch.float16: 'fp16', torch.float32: 'fp32'}


def fmt_of(x):
    return x if isinstance(x, str) else TORCH_FMT[x]


def ulp(x, fmt):
    """ulp of |x| in `fmt` ('bf16', 'fp16', 'fp32' or a torch dtype), with the subnormal floor 2^(emin - p + 1)."""
    p, emin = FORMATS[fmt_of(fmt)]
    a = x.double().abs()
    e = torch.floor(torch.log2(torch.clamp(a, min=2.0 ** (emin - 1))))
    e = torch.clamp(e, min=emin)
    return torch.exp2(e - (p - 1))


def half_ulp(x, fmt):
    return 0.5 * ulp(x, fmt)


def pair_resolution(x, fmt):
    """Resolution of a (hi, lo) pair hi = round(x), lo = round(x - hi) in `fmt`: ulp of lo, whose magnitude is at most half an ulp
    of hi.  The pair's rounding error is at most half of this."""
    return ulp(0.5 * ulp(x, fmt), fmt)


def out_round(val, pre, fmt, pair=False):
    """Half an ulp of the output format at the largest magnitude the pre-rounding value can take (|ref| + pre-rounding bound)."""
    mag = val.double().abs() + pre
    return 0.5 * (pair_resolution(mag, fmt) if pair else ulp(mag, fmt))


# ------------------------------------------------------------------ the check

def gemm_layout(bm=128, bn=128):
    def where(idx, shape):
        m, n = idx
        return f'row {m}, col {n} (row tile {m // bm} of {bm}, col tile {n // bn} of {bn})'
    return where


def attn_layout(cu_lens, heads, head_dim, rows=64):
    cl = [int(c) for c in cu_lens]

    def where(idx, shape):
        t, c = idx
        s = max(i for i in range(len(cl) - 1) if cl[i] <= t)
        r = t - cl[s]
        return f'sequence {s} (length {cl[s + 1] - cl[s]}), head {c // head_dim}, row {r} (work item {r // rows} of {rows} rows)'
    return where


def assert_bounded(got, ref64, bound, what, where=None):
    """|got - ref64| <= bound elementwise (no rms floor).  Returns max(err / bound).  On failure: the count, the worst ratio,
    its index mapped back by `where(idx, shape)` (gemm_layout / attn_layout) to row / column / tile or sequence / head / work item."""
    got = got.detach()
    ref64 = ref64.to(got.device)
    bound = bound.to(got.device).double()
    assert got.shape == ref64.shape == bound.shape, (what, got.shape, ref64.shape, bound.shape)
    g = got.double()
    assert bool(torch.isfinite(g).all()), f'{what}: non-finite output'
    err = (g - ref64.double()).abs()
    ratio = err / bound
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > 1.0:
        nbad = int((ratio > 1.0).sum())
        flat = int(ratio.argmax())
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))
        loc = where(idx, tuple(ratio.shape)) if where is not None and len(idx) == 2 else str(idx)
        raise AssertionError(f'{what}: {nbad}/{ratio.numel()} elements out of bound, worst err/bound {worst:.3g} at {loc}: '
                             f'got {float(g[idx]):.9g}, ref {float(ref64[idx]):.9g}, bound {float(bound[idx]):.3g}')
    return worst


def budget_used(got, ref64, bound, pre):
    """The share of the pre-rounding budget an output uses: max over elements of (err - output rounding term) / pre, where the output
    rounding term is bound - pre.  An element on a rounding tie sits at err / bound ~ 1 whatever its accumulation did; this says how
    much of the accumulation / epilogue terms the kernel actually needed."""
    ref = ref64.to(got.device).double()
    bound, pre = bound.to(got.device).double(), pre.to(got.device).double()
    err = (got.double() - ref).abs()
    return float((torch.clamp(err - (bound - pre), min=0.0) / pre).max())


def rounding_bias(got, ref64, pre, fmt):
    """Mean of (|got| - |ref|) / ulp over the elements whose pre-rounding bound `pre` is under 0.05 ulp: about 0 for round to
    nearest, about -0.5 for truncation.  Returns (bias, number of elements used)."""
    fmt = fmt_of(fmt)
    ref = ref64.to(got.device).double()
    u = ulp(ref, fmt)
    m = (pre.to(got.device).double() < 0.05 * u) & (ref != 0)
    n = int(m.sum())
    if n == 0:
        return 0.0, 0
    d = (got.double().abs() - ref.abs()) / u
    return float(d[m].mean()), n


# ------------------------------------------------------------------ recipes: GEMM

def dot_term(a, w, k=None):
    """fp32 accumulation of the exact products a[m, :] * w[n, :] (statistical form, C_DOT above)."""
    a, w = a.double(), w.double()
    k = a.shape[1] if k is None else k
    return C_DOT * U32 * math.sqrt(k) * torch.sqrt(torch.clamp((a * a) @ (w * w).T, min=0.0))


def gelu64(y):
    return 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))


def gelu_prime64(y):
    return 0.5 * (1.0 + torch.erf(y / math.sqrt(2.0))) + y * torch.exp(-0.5 * y * y) / math.sqrt(2.0 * math.pi)


def gelu_bound(y, pre, deg):
    """GELU epilogue (gemm.hip:945-946 in gemm_bf16_kernel, common.h:175-182 above gelu_poly): the input error through |gelu'| (|gelu''| <= 0.8 covers its change over
    the interval), plus the polynomial's stated error: 0.19 (degree 5) or 0.002 (degree 7) of half a bf16 ulp of the result, floor
    1.5e-7 |x|; plus the fma that forms max(x, 0) - |x| 2^p (one fp32 rounding)."""
    g = gelu64(y)
    poly = (0.19 if deg == 5 else 0.002) * half_ulp(g, 'bf16') + 1.5e-7 * y.abs()
    return (gelu_prime64(y).abs() + 0.8 * pre) * pre + poly + U32 * g.abs()


def gemm_reference(a, w, bias=None, epi='none', resid=None, alpha=1.0, out_fmt='bf16', gelu_deg=7, pair=False, k_eff=None):
    """float64 reference and per-element bound of C = epi(A W^T + bias) as esme_hip_gemm_bf16* computes it (plain epilogues).
    Returns (ref, bound, pre): `pre` is the bound before the output rounding (what rounding_bias filters on)."""
    a64, w64 = a.double(), w.double()
    y = a64 @ w64.T
    pre = dot_term(a64, w64, k_eff)
    if bias is not None:
        y = y + bias.double()
        pre = pre + U32 * y.abs()                           # acc + bias, one fp32 add (gemm.hip:941, gemm_bf16_kernel)
    if epi == 'none':
        val = y
    elif epi == 'gelu':
        val = gelu64(y)
        pre = gelu_bound(y, pre, gelu_deg)                  # gemm.hip:945-946, gemm_bf16_kernel
    elif epi == 'residual':
        r = resid.double()
        val = r + alpha * y
        pre = abs(alpha) * pre + U32 * (abs(alpha) * y.abs() + val.abs())     # bf(r) + alpha * o: mul and add (gemm.hip:956-957, gemm_bf16_kernel)
    else:
        raise ValueError(epi)
    return val, pre + out_round(val, pre, out_fmt, pair), pre  # pack16 / the pair split: one rounding each (gemm.hip:960-963, gemm_bf16_kernel)


def swiglu_reference(a, wa, wf, out_fmt='bf16'):
    """SwiGLU epilogue (gemm.hip:936, gemm_bf16_kernel): gate * rcp(1 + exp2(-log2(e) gate)) * fc.  Steps: the exp2 argument's fp32 product
    (relative ln2 * 2^-24 |log2(e) gate| = 2^-24 |gate| on the exponential), v_exp_f32, the add of 1, v_rcp_f32, two products.  The
    input errors propagate through |d silu / d gate| <= 1.1 and |silu(gate)|."""
    a64 = a.double()
    return swiglu_bound(a64 @ wa.double().T, a64 @ wf.double().T, dot_term(a64, wa), dot_term(a64, wf), out_fmt)


def swiglu_bound(g, f, dg, df, out_fmt='bf16'):
    """The SwiGLU epilogue of swiglu_reference on gate / fc values g, f (float64) that carry the pre-epilogue bounds dg, df: the plain GEMM's
    dot terms, or the LayerNorm-folded projection's `pre` (ln_fold_reference).  Returns (val, bound, pre)."""
    sig = torch.sigmoid(g)
    silu = g * sig
    val = silu * f
    approx = U32 * (g.abs() + 2.0) + 2 * E_TRANS + U32 * 2   # exp-arg product, add, exp, rcp, two products
    pre = (1.1 + dg) * dg * f.abs() + silu.abs() * df + dg * df + approx * val.abs()
    return val, pre + out_round(val, pre, out_fmt), pre


def ln_fold_reference(x, wprime, c1, c2, eps, sums=None, dim=None):
    """LayerNorm fold: y = rstd (acc - mean c1) + c2 with acc = x . W'[n], computed from the operands handed to the kernel -- x (the MFMA
    operand), W', c1, c2 and the fp32 partial sums {sum, sum of squares} (`sums`, (T, 2) or (nblk, T, 2); None: exact sums of x).
    Steps (gemm.hip:333-337, gemm_bf16_kernel): mean = s1 * fl(1/E) (two roundings), var = s2 * fl(1/E) - mean^2 (two products, one subtraction: the
    cancellation term 2^-24 (s2/E + mean^2), large against var when |mean| >> std -- the dc20 / outlier kinds), rstd = v_rsq_f32 of
    var + eps (one add, E_TRANS), rstd * mean (one product); the epilogue (gemm.hip:582, gemm_bf16_kernel) fma(rstd, acc, fma(-rstd mean, c1, c2)): two
    roundings, 2^-24 (|c2 - rstd mean c1| + |y|).  The accumulation term enters scaled by rstd."""
    x64 = x.double()
    E = x64.shape[1] if dim is None else dim
    if sums is None:
        s1, s2 = x64.sum(1, keepdim=True), (x64 * x64).sum(1, keepdim=True)
    else:
        sg = sums.double().reshape(-1, x64.shape[0], 2).sum(0)
        s1, s2 = sg[:, :1], sg[:, 1:]
    mean = s1 / E
    m2 = s2 / E
    var = torch.clamp(m2 - mean * mean, min=0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    c1d, c2d = c1.double(), c2.double()
    acc = x64 @ wprime.double().T
    y = rstd * (acc - mean * c1d) + c2d
    dmean = 2 * U32 * mean.abs()
    dvar = 2 * U32 * m2 + 2 * mean.abs() * dmean + U32 * mean * mean + U32 * var
    rel_rstd = 0.5 * dvar / (var + eps) + 0.5 * U32 + E_TRANS
    rm = rstd * mean * c1d
    pre = (rstd * dot_term(x64, wprime) + (y - c2d).abs() * rel_rstd + rstd * c1d.abs() * dmean
           + U32 * (rm.abs() + (c2d - rm).abs() + y.abs()))
    return y, pre


def rotary_apply64(x, cos, sin, pos):
    """x (T, H, d) float64 rotated with tables (P, d) at positions pos (T)."""
    d = x.shape[-1]
    c = cos.double()[pos.long(), : d // 2].unsqueeze(1)
    s = sin.double()[pos.long(), : d // 2].unsqueeze(1)
    lo, up = x[..., : d // 2], x[..., d // 2:]
    return torch.cat((lo * c - up * s, up * c + lo * s), dim=-1)


def rotary_bound(x, pre, cos, sin, pos, q_scale=None):
    """Rotation in fp32 with the tables in their stated type (gemm.hip:661-662 in gemm_bf16_kernel, rowops.hip:353-386 rotary_kernel): one product rounded,
    one fused -- 2^-24 (|lo c| + |up s|) + 2^-24 |result|; the input error `pre` enters through |c| + |s| <= sqrt 2; q_scale (gemm.hip:677, gemm_bf16_kernel)
    rounds once more."""
    d = x.shape[-1]
    c = cos.double()[pos.long(), : d // 2].unsqueeze(1)
    s = sin.double()[pos.long(), : d // 2].unsqueeze(1)
    lo, up = x[..., : d // 2], x[..., d // 2:]
    plo, pup = pre[..., : d // 2], pre[..., d // 2:]
    r = rotary_apply64(x, cos, sin, pos)
    e_lo = (c.abs() * plo + s.abs() * pup) + U32 * ((lo * c).abs() + (up * s).abs() + r[..., : d // 2].abs())
    e_up = (c.abs() * pup + s.abs() * plo) + U32 * ((up * c).abs() + (lo * s).abs() + r[..., d // 2:].abs())
    e = torch.cat((e_lo, e_up), dim=-1)
    if q_scale is not None:
        r = r * q_scale
        e = e * abs(q_scale) + U32 * r.abs()
    return r, e


# ------------------------------------------------------------------ recipes: attention

# relative half ulp of P's format (unit roundoff); the split-operand kernel splits P into a bf16 pair in registers (|lo| <= 2^-8 |p|,
# rounded to 2^-8 of itself: 2^-16) and leaves out Pl Vl (2^-8 |p| times 2^-8 |v|: 2^-16 of each term)
P_UNIT = {'bf16': 2.0 ** -8, 'fp16': 2.0 ** -11, 'fp32': 2.0 ** -24, 'bf16pair': 2.0 ** -16 + 2.0 ** -16}


# query rows per work item of the fixed-reference fp16 form (attn_pp64_kernel<4, true, D, true>: ROWS = NW * 64, attn.hip:687)
FIXED_REF_ITEM_ROWS = 256


def attention_reference(q, k, v, cu_lens, heads, scale, p_fmt, out_fmt, log2_units=False, fixed_ref=None, pair_out=False,
                        qk_drop=0.0, item_rows=FIXED_REF_ITEM_ROWS):
    """float64 attention of what the kernel was given, its per-element bound and the part of it before the output rounding

        u_P (C_DOT ||p o v||_2 + |o|) + (2 e_exp + 2 e_score) * sum_j p_j |v_j| + subnormal floor of P + PV accumulation + 1/l and product
        + 1/2 ulp(o)

    - u_P: P rounded to its format before the PV MFMA (attn.hip:870 pack16 in attn_pp64_kernel's pair_sum_pack, :1292 in
      attn_sb_kernel's, and the fp16 / pair forms): relative half an ulp per
      term.  The row sum l adds the UNROUNDED P (attn.hip:871, pair_sum_pack in attn_pp64_kernel; :1293 in attn_sb_kernel: no kernel
      in the library sums the rounded P), so these roundings enter the numerator only: C_DOT u_P ||p o v||_2 for
      the independent part (keys with distinct scores round independently), plus u_P |o| for the part they share (a row whose keys
      tie rounds every P alike: its error is u_P o).  Sized by test_error_bounds_cpu.py::test_c_dot_covers_p_rounding.  The worst case
      u_P sum_j p_j |v_j| would accept a bf16 P or a bf16 output in one fp16 work item of a 700-key sequence;
    - e_exp: v_exp_f32 (attn.hip:271 attn_varlen_kernel, :549 attn_split_kernel, :877-886 softmax_slot in attn_pp64_kernel),
      plus the fp32 fma that forms its argument score * c - m (2^-24 of |argument|)
      and the subtraction's own rounding;
    - e_score: fp32 accumulation of the score products (C_DOT form over d), times scale * log2(e), in log2 units -> ln 2 relative;
      the row sum and the output then see each perturbation twice (numerator and normaliser), hence the factors 2;
    - fp16 P below 2^-14 (subnormal): absolute 2^-25 per term, relative to the kernel's row sum l = sum 2^(t_j - r), r the reference
      the kernel subtracts.  Forms with a maximum: r = the row maximum (a first-tile reference is lower and only makes l larger).  The
      fixed-reference form (fixed_ref = 4, q_prescaled fp16): r = 4, unless the item_rows-row work item is redone with exact maxima
      -- the kernel's own test (attn.hip:1069-1076, attn_pp64_kernel): a row whose sum at reference 4 falls below S * 2^-14
      (S = the sequence length)
      redoes its whole work item.  Items with a row clearly under that threshold (half of it) take r = the row maximum; every other
      row r = max(4, row maximum), the larger of the two bounds (an item redone for overflow subtracts its maximum, above 4);
    - 1 / l then o * inv (attn.hip:1093-1100, attn_pp64_kernel; :314-324 attn_varlen_kernel): E_TRANS + 2^-24 relative; the
      output rounding half an ulp (pair: of the pair).
    q / k / v: (T, H*d), for a pair the sum hi + lo; qk_drop (q / k as pairs): the relative size of the Ql Kl product the pair
    kernels leave out (bf16 pairs 2^-16, fp16 pairs 2^-22), times sum |q k|, with three accumulation passes instead of one."""
    T, E = q.shape
    d = E // heads
    u_p = P_UNIT[p_fmt if isinstance(p_fmt, str) else fmt_of(p_fmt)]
    ref = torch.empty(T, E, dtype=torch.float64, device=q.device)
    bound = torch.empty_like(ref)
    log2e = 1.0 / math.log(2.0)
    cl = [int(c) for c in cu_lens]
    for s0, s1 in zip(cl[:-1], cl[1:]):
        if s1 == s0:
            continue
        qq, kk, vv = (t[s0:s1].double().view(-1, heads, d).transpose(0, 1) for t in (q, k, v))
        qd, kd = qq, kk
        s = qd @ kd.transpose(1, 2)
        # the score products' magnitude, for the statistical accumulation term: ||q_i o k_j||_2 (pair: the three passes' terms)
        sq = torch.sqrt(torch.clamp((qd * qd) @ (kd * kd).transpose(1, 2), min=0.0))
        t = s * (scale if not log2_units else 1.0) * (log2e if not log2_units else 1.0)        # scores in log2 units
        ds = (C_DOT * U32 * math.sqrt(d * (3 if qk_drop else 1)) * sq
              + qk_drop * (qd.abs() @ kd.abs().transpose(1, 2))) * (scale if not log2_units else 1.0) * (log2e if not log2_units else 1.0)
        tmax = t.max(dim=-1, keepdim=True).values
        p = torch.exp2(t - tmax)
        l = p.sum(-1, keepdim=True)
        pn = p / l
        o = pn @ vv
        mag = pn @ vv.abs()
        # per row: worst relative perturbation of any P (score error and the exp argument's rounding, in log2 units -> ln 2)
        arg = (t - tmax).abs() + t.abs()
        e_row = math.log(2.0) * (ds + 3 * U32 * arg).amax(-1, keepdim=True) + E_TRANS
        r = tmax
        if fixed_ref is not None:
            r = torch.clamp(tmax, min=fixed_ref)
            l_ref = torch.exp2(t - fixed_ref).sum(-1, keepdim=True)            # (H, L, 1): the row sums the kernel tests
            vanished = (l_ref < 0.5 * (s1 - s0) * 2.0 ** -14).squeeze(-1)
            for i0 in range(0, s1 - s0, item_rows):
                redo = vanished[:, i0:i0 + item_rows].any(-1)                  # per head
                r[redo, i0:i0 + item_rows] = tmax[redo, i0:i0 + item_rows]
        sub = torch.zeros_like(mag)
        if fmt_of(p_fmt) == 'fp16':
            lk = torch.exp2(t - r).sum(-1, keepdim=True)      # the kernel's row sum at reference r
            sub = 2.0 ** -25 * vv.abs().sum(-2, keepdim=True).expand_as(o) / lk
        pv_norm = torch.sqrt(torch.clamp((pn * pn) @ (vv * vv), min=0.0))        # ||p o v||_2 per output element
        pv = C_DOT * U32 * math.sqrt(s1 - s0) * pv_norm
        pre = u_p * (C_DOT * pv_norm + o.abs()) + 2 * e_row * mag + 2 * sub + pv + (E_TRANS + U32) * o.abs()
        ref[s0:s1] = o.transpose(0, 1).reshape(-1, E)
        bound[s0:s1] = pre.transpose(0, 1).reshape(-1, E)
    return ref, bound + out_round(ref, bound, out_fmt, pair_out), bound


# ------------------------------------------------------------------ recipes: row ops

def layernorm_reference(x, w, b, eps, out_fmt, pair=False):
    """esme_hip_layernorm* (rowops.hip:103-145, layernorm_kernel): mean = fp32 sum * (1/E), var = fp32 sum of (x - mean)^2 * (1/E), rstd = v_rsq_f32,
    y = fma((x - mean) * rstd, w, b) -- per element  |w| rstd (|x - mean| e_rel + dmean) + 2^-24 (|(x - mean) rstd w| + |y|), with
    e_rel = 1/2 dvar / var + E_TRANS (rsq) + 2^-24 (x - mean) + 2^-24 (the product with rstd); then the output rounding."""
    x64 = x.double()
    E = x64.shape[1]
    mean = x64.mean(1, keepdim=True)
    xc = x64 - mean
    var = (xc * xc).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    w64 = w.double()
    y = xc * rstd * w64 + (b.double() if b is not None else 0.0)
    dsum = C_DOT * U32 * math.sqrt(E) * torch.sqrt((x64 * x64).sum(1, keepdim=True))
    dmean = dsum / E + 2 * U32 * mean.abs()
    dss = C_DOT * U32 * math.sqrt(E) * torch.sqrt((xc ** 4).sum(1, keepdim=True)) + 2 * U32 * (xc * xc).sum(1, keepdim=True)
    dvar = dss / E + 2 * U32 * var + 2 * (xc.abs().mean(1, keepdim=True)) * dmean
    e_rel = 0.5 * dvar / (var + eps) + E_TRANS + 3 * U32
    pre = w64.abs() * rstd * (xc.abs() * e_rel + dmean) + U32 * ((xc * rstd * w64).abs() + y.abs())
    return y, pre + out_round(y, pre, out_fmt, pair), pre


def softmax_reference(x, log, out_fmt):
    """esme_hip_softmax_rows* (rowops.hip:729-753, softmax_rows_kernel and softmax_rows_f32_kernel): m = max, e = __expf(v - m) (v_exp_f32 of (v - m) log2 e: 2^-24 |v - m| on the
    argument, E_TRANS), sum in fp32 over V <= 64 terms (V 2^-24 relative), then e / sum or (v - m) - __logf(sum)."""
    x64 = x.double()
    V = x64.shape[1]
    m = x64.max(1, keepdim=True).values
    z = x64 - m
    lse = torch.logsumexp(z, 1, keepdim=True)
    if log:
        val = z - lse
        pre = U32 * z.abs() + (V * U32 + 2 * E_TRANS + U32) + E_TRANS * lse.abs() + U32 * (val.abs() + lse.abs())
    else:
        val = torch.exp(z - lse)
        pre = val * (2 * (U32 * z.abs().amax(1, keepdim=True) + E_TRANS) + V * U32 + E_TRANS + 2 * U32)
    return val, pre + out_round(val, pre, out_fmt), pre
