"""Operands of the GEMM error-bound tests, and the ledger of their worst ratios: one place for tests/test_error_bounds_gpu.py and
tests/test_gemm_persistent_bounds_gpu.py (and, on the CPU, tests/test_gemm_persistent_cpu.py).  Every builder is seeded; `dev` is where
the tensors end up ('cuda:0' by default; the generators always run on the CPU, so the values do not depend on the device)."""
import math

import torch

import error_bounds as eb

DEV = 'cuda:0'
BF = torch.bfloat16
H16 = torch.float16
BIAS_MIN_ELEMENTS = 3 * 10 ** 5          # outputs this large leave >= 10^5 elements under the 0.05-ulp filter in every recipe that calls record_bias


class Ledger:
    """Worst err / bound per family, the share of the pre-rounding budget used, the rounding bias per kernel; printed by report()."""

    def __init__(self, title):
        self.title, self.margins, self.used, self.biases = title, {}, {}, {}

    def record(self, family, ratio, used=None):
        """Keep the worst err / bound per family and, where the recipe's pre-rounding part is given, the share of it used
        (eb.budget_used: what is left once an element on a rounding tie is set aside)."""
        self.margins[family] = max(self.margins.get(family, 0.0), ratio)
        if used is not None:
            self.used[family] = max(self.used.get(family, 0.0), used)
        return ratio

    def record_bias(self, kernel, got, ref, pre, fmt, need=10 ** 5):
        """|rounding bias| < 0.05 ulp over at least `need` elements whose pre-rounding bound is under 0.05 ulp.  Fewer such elements is a
        failure, not a skip: call it only where the shape and the recipe leave enough of them (the call sites say which)."""
        bias, n = eb.rounding_bias(got, ref, pre, fmt)
        assert n >= need, f'{kernel}: only {n} elements qualify for the rounding-bias check (need {need})'
        prev = self.biases.get(kernel)
        self.biases[kernel] = bias if prev is None or abs(bias) > abs(prev[0]) else prev[0], n
        assert abs(bias) < 0.05, f'{kernel}: rounding bias {bias:+.3f} ulp over {n} elements (round to nearest gives ~0)'
        return bias, n

    def lines(self):
        out = [f'[{self.title}] worst err / bound per kernel family:']
        for k in sorted(self.margins):
            out.append(f'  {k:40s} {self.margins[k]:.3f}' + (f'   pre-rounding budget used {self.used[k]:.3f}' if k in self.used else ''))
        out.append(f'[{self.title}] rounding bias (ulp) per kernel:')
        for k in sorted(self.biases):
            out.append(f'  {k:40s} {self.biases[k][0]:+.4f}  (n = {self.biases[k][1]})')
        return out

    def report(self):
        print('\n' + '\n'.join(self.lines()))


def rnd(shape, seed, scale=1.0, dtype=BF, offset=0.0, dev=DEV):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + offset).to(dtype).to(dev)


def plain_operands(M, N, K, dev=DEV):
    """(a, w, bias, resid) of the plain / GELU / residual / SwiGLU epilogues."""
    return rnd((M, K), M + K, dev=dev), rnd((N, K), N + K, 1 / math.sqrt(K), dev=dev), rnd((N,), N, 0.5, dev=dev), rnd((M, N), 3 + M, dev=dev)


def swiglu_pack(wa, wf):
    """Gate and fc rows ((F, ...) each) interleaved in blocks of 32, as the SwiGLU epilogue reads them."""
    F = wa.shape[0]
    rest = wa.shape[1:]
    return torch.cat((wa.view(F // 32, 1, 32, *rest), wf.view(F // 32, 1, 32, *rest)), 1).reshape(2 * F, *rest).contiguous()


def ln_fold_operands(T, E, N, seed, kind, dev=DEV):
    """(x, W' = W gamma, c1, c2) of a LayerNorm-folded bf16 GEMM; `kind`: 'plain', 'dc20' (rows offset by 20) or 'outlier' (one massive channel)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, E, generator=g) * 1.5
    if kind == 'dc20':
        x = x + 20.0
    elif kind == 'outlier':
        x[:, 7] *= 60.0
    gamma = (1 + 0.1 * torch.randn(E, generator=g)).to(BF)
    beta = (0.05 * torch.randn(E, generator=g)).to(BF)
    w = (torch.randn(N, E, generator=g) * E ** -0.5).to(BF)
    b = (0.1 * torch.randn(N, generator=g)).to(BF)
    wprime = (w.double() * gamma.double()).to(BF)
    c1 = wprime.double().sum(1).float()
    c2 = (w.double() @ beta.double() + b.double()).float()
    return x.to(BF).to(dev), wprime.to(dev), c1.to(dev), c2.to(dev)


def residual_stream_operands(M, N, K, dev=DEV):
    """(a, w, bias, resid, x32) of the residual epilogue on the bf16 stream (resid) and on the fp32 stream (x32)."""
    a, w, b = rnd((M, K), 60, dev=dev), rnd((N, K), 61, 1 / math.sqrt(K), dev=dev), rnd((N,), 62, 0.5, dev=dev)
    r = rnd((M, N), 63, dev=dev)
    x32 = (torch.randn(M, N, generator=torch.Generator().manual_seed(64)) * 2).to(dev)
    return a, w, b, r, x32


def stats_reference(got, nblk):
    """stats_out: per row {sum, sum of squares} of the ROUNDED outputs `got`, fp32 partials per column block: (reference, bound) of the partials'
    sum over the blocks."""
    N = got.shape[1]
    o = got.double()
    s_ref = torch.stack((o.sum(1), (o * o).sum(1)), 1)
    sb = torch.stack((eb.C_DOT * eb.U32 * math.sqrt(N) * torch.sqrt((o * o).sum(1)) + nblk * eb.U32 * o.abs().sum(1),
                      eb.C_DOT * eb.U32 * math.sqrt(N) * torch.sqrt((o ** 4).sum(1)) + (nblk + 1) * eb.U32 * (o * o).sum(1)), 1)
    return s_ref, sb


def f16_operands(M, N, K, dev=DEV):
    """(a, w, bias) of precision 'half': fp16 activations, bf16 weights converted to fp16 (exact), bf16 bias."""
    return rnd((M, K), 70, dtype=H16, dev=dev), rnd((N, K), 71, 1 / math.sqrt(K), dev=dev).to(H16), rnd((N,), 72, 0.5, dev=dev)


def f16_ln_fold_operands(T, E, N, seed, sel):
    """Precision 'half' LayerNorm-folded projection over a stream with massive channels `sel` (int32, ascending): CPU tensors
    (x32 (T, E) fp32 stream, W' fp16 (N, E), W' with the extension K-tile [W' | W'[:, sel] | 0] (N, E + 64), c1, c2)."""
    g = torch.Generator().manual_seed(seed)
    x32 = torch.randn(T, E, generator=g) * 1.5
    x32[:, sel.long()] *= 200.0
    gamma = (1 + 0.1 * torch.randn(E, generator=g)).to(BF)
    beta = (0.05 * torch.randn(E, generator=g)).to(BF)
    w = (torch.randn(N, E, generator=g) * E ** -0.5).to(BF)
    b = (0.1 * torch.randn(N, generator=g)).to(BF)
    wp = (w.double() * gamma.double()).to(H16)
    wext = torch.cat((wp, wp[:, sel.long()], torch.zeros(N, 64 - len(sel), dtype=H16)), 1).contiguous()
    c1 = wp.double().sum(1).float()
    c2 = (w.double() @ beta.double() + b.double()).float()
    return x32, wp, wext, c1, c2
