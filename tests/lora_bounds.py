"""Float64 reference and per-element bound for the LoRA path (esme/lora.py, csrc/lora.hip), in the manner of attn_pool_bounds.py.

The reference's data flow for a wrapped projection (its esme/lora.py: LoRA.forward / lora_forward; esme/attention.py: _qkv), stated in
float64:
        y = LN(x) W^T + b + sum_n s B_n (A_n LN(x)),        s = alpha / rank
with the delta entering BEFORE ESM-C's q / k LayerNorm and before rotary.  The package computes it as ONE LayerNorm-folded GEMM over an
extension K-tile:
        y = rstd ([x | u] [W' | sB]^T - mean c1) + c2,      u = bf16((x - mean) (gamma A)^T + sd (A beta)),  sd = sqrt(var + eps).
`qkv_reference` evaluates the first form in float64 on the operands the kernels are handed for the base part (W' = bf16(W gamma), c1, c2:
what tests/error_bounds.py::ln_fold_reference judges the base GEMM against) and on the ORIGINAL A, B, gamma, beta, s for the adapters.
The bound is the sum of the new path's rounding steps:
  [fold]    everything ln_fold_reference prices, over K + X columns (dot_term over the extended row, statistics, epilogue);
  [A']      A' = bf16(gamma A): 2^-9 relative per element, through |x - mean| and |sB|;
  [u]       esme_hip_lora_down's own bound (down_reference: fp32 accumulation, the statistics, two fmas) and the rounding of u to
            bf16 (2^-9 |u|), through |sB|;
  [sB]      sB = bf16(s B): 2^-9 relative, through |u|;
  [out]     the epilogue's rounding of y to bf16.
The three adapter terms enter scaled by rstd, like the accumulator.  `emulate_qkv` restates the kernel path in fp32 / bf16 on the CPU and
can inject the defects a review would look for; the bound must accept the faithful emulation and reject each of them.
"""
import math

import torch

import error_bounds as eb

U_BF = 2.0 ** -9        # bf16 unit roundoff (half an ulp relative)


def _bf(t):
    return t.to(torch.bfloat16)


def ext_width(rows):
    return (rows + 63) // 64 * 64


def stats64(x, dim=None):
    x64 = x.double()
    E = x64.shape[1] if dim is None else dim
    s1, s2 = x64.sum(1, keepdim=True), (x64 * x64).sum(1, keepdim=True)
    mean = s1 / E
    var = torch.clamp(s2 / E - mean * mean, min=0.0)
    return torch.stack((s1[:, 0], s2[:, 0]), dim=1).unsqueeze(0), mean, var


def fold(W, bias, gamma, beta):
    """(W' bf16, c1 f32, c2 f32) as esme.attention._fold_layernorm forms them."""
    wf = _bf(W.float() * gamma.float().unsqueeze(0))
    c1 = wf.float().sum(1)
    c2 = torch.zeros(W.shape[0])
    if beta is not None:
        c2 = c2 + W.float() @ beta.float()
    if bias is not None:
        c2 = c2 + bias.float()
    return wf, c1, c2


def stack(adapters, names, projs, E, s):
    """Stacked operands of one QKV GEMM: A (R, E) bf16 and the placed s B (3E, R) float64, projection blocks in q, k, v order and inside a
    projection in `names` order (esme.attention._lora_weights).  adapters[name][proj] = (A (r, E), B (E, r))."""
    rows, cols, o = [], [], 0
    for i, p in enumerate(('q', 'k', 'v')):
        if p not in projs:
            continue
        for n in names:
            A, B = adapters[n][p]
            rows.append(A)
            blk = torch.zeros(3 * E, A.shape[0], dtype=torch.float64)
            blk[i * E:(i + 1) * E] = B.double() * s
            cols.append(blk)
    return torch.cat(rows, 0), torch.cat(cols, 1)


def down_reference(x, A, sums=None, dim=None, eps=1e-5, c1=None, bA=None):
    """float64 reference and per-element bound of esme_hip_lora_down[_ln] on the operands handed to the kernel: x, A bf16; LN form: the fp32
    partial sums, c1, bA.  Steps (lora.hip): fp32 MFMA accumulation (dot_term); LN form: mean = s1 * fl(1 / E) (two roundings), var = s2 *
    fl(1 / E) - mean^2 (cancellation term as in ln_fold_reference), sd = sqrtf(var + eps) (one add, a correctly rounded root), then
    fma(sd, bA, fma(-mean, c1, acc)): two roundings.  One rounding to bf16.  Returns (u64, bound, pre)."""
    x64, A64 = x.double(), A.double()
    acc = x64 @ A64.T
    pre = eb.dot_term(x64, A64)
    if c1 is None:
        return acc, pre + eb.out_round(acc, pre, 'bf16'), pre
    E = x64.shape[1] if dim is None else dim
    if sums is None:
        sums = stats64(x, E)[0]
    sg = sums.double().reshape(-1, x64.shape[0], 2).sum(0)
    mean, m2 = sg[:, :1] / E, sg[:, 1:] / E
    var = torch.clamp(m2 - mean * mean, min=0.0)
    sd = torch.sqrt(var + eps)
    c1d, bd = c1.double(), bA.double()
    inner = acc - mean * c1d
    u = inner + sd * bd
    dmean = 2 * eb.U32 * mean.abs()
    dvar = 2 * eb.U32 * m2 + 2 * mean.abs() * dmean + eb.U32 * mean * mean + eb.U32 * var
    rel_sd = 0.5 * dvar / (var + eps) + 1.5 * eb.U32
    pre = pre + c1d.abs() * dmean + (sd * bd).abs() * rel_sd + eb.U32 * (inner.abs() + u.abs())
    return u, pre + eb.out_round(u, pre, 'bf16'), pre


def qkv_reference(x, W, bias, gamma, beta, eps, adapters, names, projs, s, sums=None):
    """(ref64 (T, 3E), bound, pre, parts) of the fused QKV projection with the adapters `names` on `projs` (module docstring)."""
    T, E = x.shape
    wf, c1, c2 = fold(W, bias, gamma, beta)
    if sums is None:
        sums = stats64(x)[0]
    sg = sums.double().reshape(-1, T, 2).sum(0)
    mean = sg[:, :1] / E
    var = torch.clamp(sg[:, 1:] / E - mean * mean, min=0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    if not names or not projs:
        y, pre = eb.ln_fold_reference(x, wf, c1, c2, eps, sums=sums, dim=E)
        return y, pre + eb.out_round(y, pre, 'bf16'), pre, None
    A, sB = stack(adapters, names, projs, E, s)
    gA = A.double() * gamma.double().unsqueeze(0)                          # exact gamma * A
    bA = A.double() @ (beta.double() if beta is not None else torch.zeros(E, dtype=torch.float64))
    xc = x.double() - mean
    u = xc @ gA.T + torch.sqrt(var + eps) * bA                             # = LN(x) A^T / rstd
    y, pre = eb.ln_fold_reference(torch.cat((x.double(), u), 1), torch.cat((wf.double(), sB), 1), c1, c2, eps, sums=sums, dim=E)      # [fold]
    Ap = _bf(A.float() * gamma.float().unsqueeze(0))
    _, _, pre_u = down_reference(x, Ap, sums, E, eps, Ap.float().sum(1), bA.float())
    absB = sB.abs().T
    t_a = (xc.abs() @ (gA.abs().T * U_BF)) @ absB                          # [A']
    t_u = (U_BF * u.abs() + pre_u) @ absB                                  # [u]
    t_b = U_BF * (u.abs() @ absB)                                          # [sB]
    pre = pre + rstd * (t_a + t_u + t_b)
    return y, pre + eb.out_round(y, pre, 'bf16'), pre, {'u': u, 'rstd': rstd}


def emulate_qkv(x, W, bias, gamma, beta, eps, adapters, names, projs, s, defect=None, stale=None):
    """fp32 / bf16 emulation of esme_hip_lora_down_ln + the LayerNorm-folded GEMM over the extension tile; returns bf16 (T, 3E).
    `defect`: None, 'no_scaling' (s = 1), 'inv_scaling' (rank / alpha), 'swap_qv' (the B blocks of q and v exchanged), 'drop_key' (the key
    adapter left out), 'no_beta' (the beta A^T term dropped); `stale`: adapters whose (older) lora_B is used instead."""
    T, E = x.shape
    wf, c1, c2 = fold(W, bias, gamma, beta)
    x32 = x.float()
    s1, s2 = x32.sum(1, keepdim=True), (x32 * x32).sum(1, keepdim=True)
    inv = torch.tensor(1.0 / E, dtype=torch.float32)
    mean = s1 * inv
    var = torch.clamp(s2 * inv - mean * mean, min=0.0) + torch.tensor(eps, dtype=torch.float32)
    rstd, sd = torch.rsqrt(var), torch.sqrt(var)
    if defect == 'no_scaling':
        s = 1.0
    elif defect == 'inv_scaling':
        s = 1.0 / s
    if defect == 'drop_key':
        projs = tuple(p for p in projs if p != 'k')
    src = stale if stale is not None else adapters
    if defect == 'swap_qv':
        src = {n: {**src[n], 'q': (src[n]['q'][0], src[n]['v'][1]), 'v': (src[n]['v'][0], src[n]['q'][1])} for n in src}
    if names and projs:
        A, sB = stack(src, names, projs, E, s)
        Ap = _bf(A.float() * gamma.float().unsqueeze(0))
        c1A = Ap.float().sum(1)
        bA = A.float() @ beta.float() if (beta is not None and defect != 'no_beta') else torch.zeros(A.shape[0])
        acc_u = (x.double() @ Ap.double().T).float()
        u = _bf(sd * bA + (acc_u - mean * c1A))
        X = ext_width(A.shape[0])
        xe = torch.cat((x.double(), u.double(), torch.zeros(T, X - u.shape[1], dtype=torch.float64)), 1)
        we = torch.cat((wf.double(), _bf(sB.float()).double(), torch.zeros(3 * E, X - u.shape[1], dtype=torch.float64)), 1)
    else:
        xe, we = x.double(), wf.double()
    acc = (xe @ we.T).float()
    return _bf(rstd * acc + (c2 - (rstd * mean) * c1))


def delta64(x, gamma, beta, eps, adapters, names, projs, s):
    """The exact adapter contribution sum_n s B_n A_n LN(x) (T, 3E) in float64."""
    _, mean, var = stats64(x)
    h = (x.double() - mean) / torch.sqrt(var + eps) * gamma.double() + (beta.double() if beta is not None else 0.0)
    A, sB = stack(adapters, names, projs, x.shape[1], s)
    return (h @ A.double().T) @ sB.T


def qln_reference(q, pre, w, b, eps):
    """ESM-C's q / k LayerNorm over the full width applied to a value known to `pre` per element: (LN64(q), bound).  First order,
    d LN_i = gamma_i / sigma (dq_i - mean(dq) - xhat_i mean(xhat dq)), so |d LN_i| <= |gamma_i| / sigma (e_i + mean(e) + |xhat_i| mean(|xhat| e));
    5 % on top for the second order (e << sigma), 8 fp32 roundings of the kernel's own arithmetic, and the output rounding to bf16."""
    q64 = q.double()
    mu = q64.mean(1, keepdim=True)
    sig = torch.sqrt(((q64 - mu) ** 2).mean(1, keepdim=True) + eps)
    xh = (q64 - mu) / sig
    val = xh * w.double() + (b.double() if b is not None else 0.0)
    e = pre.double()
    lin = w.double().abs() / sig * (e + e.mean(1, keepdim=True) + xh.abs() * (xh.abs() * e).mean(1, keepdim=True))
    p = 1.05 * lin + 8 * eb.U32 * (val.abs() + xh.abs() * w.double().abs())
    return val, p + eb.out_round(val, p, 'bf16')


def rotary_tables(max_len, d, dtype=torch.bfloat16):
    inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2, dtype=torch.float64) / d))
    ang = torch.arange(max_len, dtype=torch.float64).unsqueeze(1) * inv.unsqueeze(0)
    return torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)
