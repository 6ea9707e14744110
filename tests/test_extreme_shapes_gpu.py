"""Shapes past the limits the rest of the suite stays inside: more than 65 535 sequences in one batch (the attention kernels that
take the sequence from grid z launch in chunks), activations of more than 2^31 elements (and 2^32 bytes), and a 35 000-residue
sequence through the whole forward (rotary tables grown past 32 768, every attention form).

Each case checks a HIP result against a plain high-precision reference of the same operation, at the tolerance the form already
has elsewhere in the suite (tests/test_hip_kernels.py, test_half_gpu.py, test_exact_gpu.py, test_attn_qp16_gpu.py,
test_half_robust_gpu.py, test_model_gpu.py), and that a sequence's rows do not depend on what it is packed with, bit for bit.
References that would not fit the CPU in reasonable time (float64 attention over 70 000 sequences, a 35 000-residue forward) run the
same math on the GPU with torch."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_util import rel_fro
from oracle import esm_oracle as O
from esme import synthetic as syn
from test_fullsize_gpu import load
from test_hip_kernels import check
from test_model_gpu import assert_parity, build

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H16 = torch.float16
LOG2E = 1.4426950408889634
GRID_Z = 65535


@pytest.fixture(autouse=True)
def _threads_and_memory():
    torch.set_num_threads(16)
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def gpu_randn(shape, seed, dtype, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV) * scale).to(dtype)


# ------------------------------------------------------------------ many sequences: attention kernels

def many_lengths(seed=0):
    """70 000 sequences of 1 to 8 residues between two of 300 (max_len spans several query tiles; the last one has index >= 65 535)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [300] + rng.integers(1, 9, size=70000).tolist() + [300]


def grouped_attention(q, k, v, lengths, cu, H, d, scale):
    """float64 softmax(q k^T * scale) v per sequence, the sequences of one length batched together (q, k, v: (T, H*d) float64 on the GPU)."""
    T, E = q.shape
    out = torch.empty(T, E, dtype=torch.float64, device=q.device)
    lens = torch.tensor(lengths)
    starts = cu[:-1].long()
    for n in lens.unique().tolist():
        idx = (lens == n).nonzero().flatten()
        rows = (starts[idx].view(-1, 1) + torch.arange(n).view(1, -1)).to(q.device)            # (m, n)
        qs, ks, vs = (t[rows].view(-1, n, H, d).transpose(1, 2) for t in (q, k, v))            # (m, H, n, d)
        p = torch.softmax(qs @ ks.transpose(-1, -2) * scale, dim=-1)
        out[rows] = (p @ vs).transpose(1, 2).reshape(-1, n, E)
    return out


# form -> head dims; every form is one attention entry point (and, through the options, kernel) at the tolerance its own tests use
MANY_CASES = [('bf16', 16), ('bf16', 32), ('bf16', 64), ('bf16', 128),
              ('bf16_v1', 64), ('bf16_v1', 32), ('bf16_v2', 64), ('bf16_v2', 32),
              ('f16', 16), ('f16', 64), ('f16_v1', 64), ('f16_qp', 64), ('f16_qp', 32),
              ('exact', 16), ('exact', 64),
              ('split', 16), ('split', 64), ('split', 128),
              ('qkpair', 16), ('qkpair', 64), ('qkpair_v2', 64)]


def _run_form(form, x, cu, max_len, H, d):
    """x: the form's packed input on the GPU; returns the output as (T, E) float64 (pairs joined)."""
    from esme import _hip
    E = H * d
    if form.startswith('split'):
        o = _hip.attn_varlen_split(x, cu, max_len, H, d, d ** -0.5)
        return o[:, :E].double() + o[:, E:].double()
    if form.startswith('qkpair'):
        with _hip.attn_options(variant=2 if form.endswith('_v2') else 0):
            return _hip.attn_varlen_qkpair(x, cu, max_len, H, d, d ** -0.5).double()
    variant = {'_v1': 1, '_v2': 2}.get(form[-3:], 0)
    with _hip.attn_options(variant=variant):
        return _hip.attn_varlen(x[:, :E], x[:, E:2 * E], x[:, 2 * E:3 * E], cu, max_len, H, exact=form == 'exact',
                                q_prescaled=form == 'f16_qp').double()


@pytest.mark.parametrize('form,d', MANY_CASES)
def test_attention_more_than_65535_sequences(form, d):
    """B = 70 002: every attention entry point accepts it, every row matches float64, and the sequences around the grid-z boundary of
    the chunked launches (65 534 .. 65 540) and the last one equal the same sequences run as a batch of their own."""
    lengths = many_lengths()
    B, T = len(lengths), sum(lengths)
    H = {16: 4, 32: 2, 64: 2, 128: 1}[d]
    E = H * d
    cu = syn.cu_lens_of(lengths).to(DEV)
    max_len = max(lengths)
    seed = 1000 + d + len(form)
    scale = d ** -0.5
    if form.startswith('split'):
        xf = gpu_randn((T, 3 * E), seed, torch.float32, 1.5)
        hi = xf.to(torch.bfloat16)
        x = torch.cat((hi, (xf - hi.float()).to(torch.bfloat16)), dim=1).contiguous()
        xd = x[:, :3 * E].double() + x[:, 3 * E:].double()
        qd, kd, vd = xd[:, :E], xd[:, E:2 * E], xd[:, 2 * E:]
    elif form.startswith('qkpair'):
        q, k, v = (gpu_randn((T, E), seed + i, torch.float32, s) for i, s in enumerate((2.0, 2.0, 1.0)))
        qh, kh = q.to(H16), k.to(H16)
        x = torch.cat((qh, kh, v.to(H16), (q - qh.float()).to(H16), (k - kh.float()).to(H16)), dim=1).contiguous()
        qd, kd, vd = x[:, :E].double() + x[:, 3 * E:4 * E].double(), x[:, E:2 * E].double() + x[:, 4 * E:].double(), x[:, 2 * E:3 * E].double()
    elif form.startswith('f16'):
        x = gpu_randn((T, 3 * E), seed, H16)
        if form == 'f16_qp':                     # q carries softmax_scale * log2(e): scores in log2 units
            x[:, :E] = (x[:, :E].float() * (scale * LOG2E)).to(H16)
            scale = 1.0 / LOG2E
        qd, kd, vd = (x[:, i * E:(i + 1) * E].double() for i in range(3))
    else:
        x = gpu_randn((T, 3 * E), seed, torch.bfloat16)
        qd, kd, vd = (x[:, i * E:(i + 1) * E].double() for i in range(3))
    got = _run_form(form, x, cu, max_len, H, d)
    torch.cuda.synchronize()
    ref = grouped_attention(qd, kd, vd, lengths, cu.cpu(), H, d, scale)
    del qd, kd, vd
    assert torch.isfinite(got).all(), form
    if form.startswith(('bf16', 'exact')):
        check(got.float(), ref.float(), rtol=2.0 ** -6, atol_scale=2.0 ** -6, what=f'attention {form} d{d} B={B}')
    else:
        e = rel(got, ref)
        print(f'\n[attn {form} d={d} B={B}] rel {e:.2e}')
        assert e <= (2e-5 if form.startswith('split') else 6e-4), (form, d, e)
    # alone == packed, bit for bit, across the chunk boundary of the grid-z launches
    cul = cu.tolist()
    picks = list(range(GRID_Z - 1, GRID_Z + 6)) + [B - 1]
    rows = torch.cat([torch.arange(cul[i], cul[i + 1]) for i in picks]).to(DEV)
    sub_len = [lengths[i] for i in picks]
    alone = _run_form(form, x[rows].contiguous(), syn.cu_lens_of(sub_len).to(DEV), max(sub_len), H, d)
    assert torch.equal(alone, got[rows]), f'{form} d{d}: sequences {picks} differ alone and packed'


# ------------------------------------------------------------------ many sequences: whole models

def peptides(n=70000, seed=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(3, 9, size=n).tolist()


MANY_MODELS = {'esm2_8m': 2, 'esm2_650m': 1, 'esmc_300m': 1}         # (8M: head dim 16, the generic kernel; 650M: 64, ping-pong; ESM-C: qk_norm_rotary)
PRECISIONS = [('fast', None), ('high', None), ('half', None), ('half', True), ('exact', None)]


@pytest.mark.parametrize('name', list(MANY_MODELS))
def test_model_more_than_65535_peptides(name):
    """70 000 peptides of 3 to 8 residues (~385 000 tokens) in every precision: sequences at both ends and around the grid-z boundary,
    plus 40 seeded picks, against the fp32 / bf16 oracle on those sequences alone, and bit-equal to the same sequences run alone."""
    model, w, H = load(name, L=MANY_MODELS[name], seed=5)
    lengths = peptides()
    B = len(lengths)
    tokens, cu = syn.random_tokens(lengths, seed=6), syn.cu_lens_of(lengths)
    ml = max(lengths)
    rng = np.random.Generator(np.random.PCG64(7))
    picks = sorted({0, 1, GRID_Z - 1, GRID_Z, GRID_Z + 1, B - 1} | set(rng.integers(0, B, size=40).tolist()))
    cul = cu.tolist()
    sub_t = torch.cat([tokens[cul[i]:cul[i + 1]] for i in picks])
    sub_len = [lengths[i] for i in picks]
    sub_cu = syn.cu_lens_of(sub_len)
    ref32 = O.forward_logits(w, H, sub_t, sub_cu, max(sub_len), dtype=torch.float32)
    refbf = O.forward_logits(w, H, sub_t, sub_cu, max(sub_len), dtype=torch.bfloat16)
    rows = torch.cat([torch.arange(cul[i], cul[i + 1]) for i in picks]).to(DEV)
    td, cd = tokens.to(DEV), cu.to(DEV)
    for mode, robust in PRECISIONS:
        model.set_precision(mode, robust=robust)
        what = f'{name} x {MANY_MODELS[name]} layers, B={B}, precision {mode}' + (' robust' if robust else '')
        out = model(td, (cd, ml))
        torch.cuda.synchronize()
        assert out.shape == (tokens.numel(), model.vocab_size) and torch.isfinite(out.float()).all(), what
        got = out[rows]
        assert_parity(got, ref32, refbf, what)
        if mode in ('half', 'exact'):                 # these modes' own bar against the fp32 forward
            assert rel_fro(got.float().cpu(), ref32) <= 1e-3, what
        alone = model(sub_t.to(DEV), (sub_cu.to(DEV), max(sub_len)))
        assert torch.equal(alone, got), f'{what}: packed rows differ from the same sequences run alone'
        del out
    model.set_precision('fast', robust='auto')
    # the mean pool over the same 70 000 sequences vs a float64 segment mean
    from esme.pooling import PartitionMeanPool
    rep = model.forward_representation(td, (cd, ml))
    pooled = PartitionMeanPool()(rep, cd)
    seg = torch.repeat_interleave(torch.arange(B, device=DEV), torch.tensor(lengths, device=DEV))
    ref = torch.zeros(B, rep.shape[1], dtype=torch.float64, device=DEV).index_add_(0, seg, rep.double())
    ref /= torch.tensor(lengths, dtype=torch.float64, device=DEV).view(-1, 1)
    check(pooled.float(), ref.float(), what=f'{name} PartitionMeanPool over B={B}')


@pytest.mark.parametrize('mode', ['fast', 'half', 'exact'])
def test_c_forward_entry_equals_module_path_past_65535_sequences(mode):
    """The one-call C forward issues the same launches as the module path on a batch of 70 000 peptides (ESM2-8M geometry: the
    chunked generic attention kernel), bit for bit."""
    model, _, _ = load('esm2_8m', L=2, seed=5)
    assert model._c_forward_ok()
    lengths = peptides(seed=8)
    tokens, cu, ml = syn.random_tokens(lengths, seed=9).to(DEV), syn.cu_lens_of(lengths).to(DEV), max(lengths)
    model.set_precision(mode)
    keep = type(model).c_forward
    try:
        type(model).c_forward = True
        a = model(tokens, (cu, ml))
        type(model).c_forward = False
        b = model(tokens, (cu, ml))
    finally:
        type(model).c_forward = keep
    assert torch.equal(a, b), mode


# ------------------------------------------------------------------ more than 2^31 elements

TILE = 256


def crossing_rows(M, widths):
    """Row blocks to check in an (M, W) tensor: the first tile, the tiles that hold element 2^30 / 2^31 / 2^32 of each width (byte 2^32 of
    4- / 2- / 1-byte data) and the last partial tile."""
    starts = {0, (M - 1) // TILE * TILE}
    for W in widths:
        for e in (1 << 30, 1 << 31, 1 << 32):
            r = e // W
            if r < M:
                starts |= {r // TILE * TILE, max(r // TILE * TILE - TILE, 0)}
    return torch.cat([torch.arange(s, min(s + TILE, M)) for s in sorted(starts)])


def test_gemm_output_past_2_31_elements():
    """C = 430 000 x 5 120 (2.2e9 elements, 4.4 GB) in each bf16 epilogue: bias, GELU, residual, SwiGLU; checked against fp32 on the
    row blocks around element 2^31 of C and at both ends."""
    from esme import _hip
    M, N, K = 430000, 5120, 1280
    assert M * N > 1 << 31
    a = gpu_randn((M, K), 1, torch.bfloat16)
    w = gpu_randn((N, K), 2, torch.bfloat16, 1 / math.sqrt(K))
    b = gpu_randn((N,), 3, torch.bfloat16, 0.1)
    rows = crossing_rows(M, [N]).to(DEV)
    lin = a[rows].float() @ w.float().T + b.float()
    got = _hip.gemm(a, w, b)
    check(got[rows], lin, what='gemm bias, C > 2^31 elements')
    got = _hip.gemm(a, w, b, _hip.EPI_GELU, out=got)
    check(got[rows], F.gelu(lin), what='gemm GELU, C > 2^31 elements')
    r = gpu_randn((M, N), 4, torch.bfloat16)
    r_rows = r[rows].float()
    _hip.gemm(a, w, b, _hip.EPI_RESIDUAL, resid=r, alpha=0.75, out=r)            # in place, as the forward does
    check(r[rows], r_rows + 0.75 * lin, what='gemm residual, C > 2^31 elements')
    del r, got
    torch.cuda.empty_cache()
    # SwiGLU over the interleaved weight: the packed product is 430 000 x 6 144 (ESM-C 600M's up-projection)
    Fw = 3072
    wa, wf = gpu_randn((Fw, K), 5, torch.bfloat16, 1 / math.sqrt(K)), gpu_randn((Fw, K), 6, torch.bfloat16, 1 / math.sqrt(K))
    packed = torch.cat((wa.view(Fw // 32, 1, 32, K), wf.view(Fw // 32, 1, 32, K)), 1).reshape(2 * Fw, K).contiguous()
    rows = crossing_rows(M, [Fw, 2 * Fw]).to(DEV)
    got = _hip.gemm(a, packed, None, _hip.EPI_SWIGLU)
    ref = F.silu(a[rows].float() @ wa.float().T) * (a[rows].float() @ wf.float().T)
    check(got[rows], ref, what='gemm SwiGLU, packed product > 2^31 elements')


def test_gemm_operand_past_2_31_elements():
    """A = 430 000 x 5 120 (the FFN-down operand at 650M width): A itself holds more than 2^31 elements."""
    from esme import _hip
    M, N, K = 430000, 1280, 5120
    a = gpu_randn((M, K), 11, torch.bfloat16)
    w = gpu_randn((N, K), 12, torch.bfloat16, 1 / math.sqrt(K))
    b = gpu_randn((N,), 13, torch.bfloat16, 0.1)
    rows = crossing_rows(M, [K, N]).to(DEV)
    got = _hip.gemm(a, w, b)
    check(got[rows], a[rows].float() @ w.float().T + b.float(), what='gemm, A > 2^31 elements')


def test_row_ops_past_2_31_elements():
    """Row operations at ESM2-15B width (E = 5 120) on 430 000 rows: LayerNorm, gather_rows and the stand-alone rotary."""
    from esme import _hip
    T, E, H = 430000, 5120, 40
    d = E // H
    rows = crossing_rows(T, [E, 2 * E]).to(DEV)
    x = gpu_randn((T, E), 21, torch.bfloat16, 2.0)
    wln = (1 + 0.1 * gpu_randn((E,), 22, torch.float32)).to(torch.bfloat16)
    bln = gpu_randn((E,), 23, torch.bfloat16, 0.1)
    y = _hip.layernorm(x, wln, bln)
    check(y[rows], F.layer_norm(x[rows].float(), (E,), wln.float(), bln.float(), 1e-5), what='layernorm, T x E > 2^31')
    del y
    idx = torch.flip(torch.arange(T, device=DEV), [0])
    idx[::7] = torch.arange(0, T, 7, device=DEV) % 1000
    g = _hip.gather_rows(x, idx)
    assert torch.equal(g[rows], x[idx[rows]]) and torch.equal(g[-1000:], x[idx[-1000:]])
    del g, x
    torch.cuda.empty_cache()
    # rotary on q / k of a (T, 2E) buffer: 500-residue sequences (+ a remainder)
    lengths = [500] * (T // 500)
    cu = syn.cu_lens_of(lengths)
    qk = gpu_randn((T, 2 * E), 24, torch.bfloat16)
    before = qk[rows].float()
    cos, sin = O.rotary_tables(500, d, torch.bfloat16)
    pos, _ = _hip.seq_positions(cu.to(DEV), T)
    _hip.rotary_(qk[:, :E], qk[:, E:], cos.to(DEV), sin.to(DEV), pos, H)
    p = O.culen_positions(cu)[rows.cpu()]
    for i, what in ((0, 'q'), (1, 'k')):
        ref = O.apply_rotary(before[:, i * E:(i + 1) * E].cpu().view(-1, H, d), cos.float(), sin.float(), p).view(-1, E)
        check(qk[rows, i * E:(i + 1) * E], ref, what=f'rotary {what}, (T, 2E) > 2^31 elements')


def long_batch(T, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    lengths = []
    while sum(lengths) < T:
        lengths.append(int(rng.integers(400, 601)))
    lengths[-1] -= sum(lengths) - T
    return lengths


@pytest.mark.parametrize('name,T,widths', [
    ('esm2_650m', 430000, lambda E: [4 * E, 8 * E, 6 * E, 3 * E, 2 * E]),      # FFN-up; its pair ('exact'); the q/k/v pair; q/k/v; the stream pair
    ('esmc_600m', 360000, lambda E: [2 * syn.swiglu_width(E), 4 * syn.swiglu_width(E), 6 * E, 3 * E, 2 * E]),
])
def test_model_activations_past_2_31_elements(name, T, widths):
    """One layer at T tokens of 400- to 600-residue sequences, where the FFN up-projection (and in 'half' / 'exact' the doubled pair buffers)
    pass 2^31 elements: the first and last sequences and those holding each crossing row vs the oracle, and bit-equal alone."""
    model, w, H = load(name, L=1, seed=2)
    E = syn.MODEL_ZOO[name][2]
    lengths = long_batch(T, seed=4)
    tokens, cu = syn.random_tokens(lengths, seed=5), syn.cu_lens_of(lengths)
    cul = np.asarray(cu.tolist())
    cross = [min(e // W, T - 1) for W in widths(E) for e in (1 << 31,) if e // W < T]
    picks = sorted({0, len(lengths) - 1} | {int(np.searchsorted(cul, r, side='right') - 1) for r in cross})
    sub_t = torch.cat([tokens[cul[i]:cul[i + 1]] for i in picks])
    sub_len = [lengths[i] for i in picks]
    sub_cu = syn.cu_lens_of(sub_len)
    ref32 = O.forward_logits(w, H, sub_t, sub_cu, max(sub_len), dtype=torch.float32)
    refbf = O.forward_logits(w, H, sub_t, sub_cu, max(sub_len), dtype=torch.bfloat16)
    rows = torch.cat([torch.arange(cul[i], cul[i + 1]) for i in picks]).to(DEV)
    td, cd = tokens.to(DEV), cu.to(DEV)
    for mode in ('fast', 'half', 'exact'):
        model.set_precision(mode)
        what = f'{name} x 1 layer, T={T}, precision {mode}, sequences {picks}'
        out = model(td, (cd, max(lengths)))
        torch.cuda.synchronize()
        got = out[rows]
        del out
        torch.cuda.empty_cache()
        assert_parity(got, ref32, refbf, what)
        if mode != 'fast':
            assert rel_fro(got.float().cpu(), ref32) <= 1e-3, what
        alone = model(sub_t.to(DEV), (sub_cu.to(DEV), max(sub_len)))
        assert torch.equal(alone, got), f'{what}: packed rows differ from the same sequences run alone'
    model.set_precision('fast')


# ------------------------------------------------------------------ a 35 000-residue sequence through forward

def chunked_attention(q, k, v, cu, H, scale, block=512):
    """float64 attention per sequence, over query blocks (a 35 000^2 score matrix per head would not fit)."""
    T, E = q.shape
    d = E // H
    out = torch.empty(T, E, dtype=q.dtype, device=q.device)
    cul = cu.tolist()
    for s0, s1 in zip(cul[:-1], cul[1:]):
        ks, vs = (t[s0:s1].double().view(-1, H, d).transpose(0, 1) for t in (k, v))
        for b0 in range(s0, s1, block):
            b1 = min(b0 + block, s1)
            qs = q[b0:b1].double().view(-1, H, d).transpose(0, 1)
            p = torch.softmax(qs @ ks.transpose(1, 2) * scale, dim=-1)
            out[b0:b1] = (p @ vs).transpose(0, 1).reshape(-1, E).to(q.dtype)
    return out


def gpu_oracle_logits(w, H, tokens, cu, max_len, dtype):
    """oracle/esm_oracle.py's forward_logits on the GPU: the same blocks (the linear layers in `dtype`), attention in float64 over
    query blocks."""
    kind, n_layers, E = O._cfg_of(w)
    wd = {k: v.to(DEV) for k, v in w.items()}
    tokens, cu = tokens.to(DEV), cu.to(DEV)
    s = math.sqrt(n_layers / 36) if kind == 'esmc' else 1.0
    d = E // H
    cos, sin = (t.to(DEV) for t in O.rotary_tables(max_len, d, dtype))
    pos = O.culen_positions(cu.cpu()).to(DEV)
    x = O.embedding(wd, tokens, kind, dtype)
    for i in range(n_layers):
        p = f'layers.{i}.self_attn.'
        g = lambda n: wd[p + n].to(dtype) if (p + n) in wd else None
        h = O._ln(x, g('norm.weight'), g('norm.bias'))
        q, k, v = (F.linear(h, g(f'{n}.weight'), g(f'{n}.bias')) for n in 'qkv')
        if kind == 'esmc':
            q, k = O._ln(q, g('layernorm_q.weight')), O._ln(k, g('layernorm_k.weight'))
        T = x.shape[0]
        q, k = (O.apply_rotary(t.view(T, H, d), cos, sin, pos).reshape(T, E) for t in (q, k))
        a = chunked_attention(q, k, v, cu, H, d ** -0.5)
        x = x + F.linear(a, g('out.weight'), g('out.bias')) / s
        x = x + O.ffn_block(wd, i, x, kind, dtype) / s
    b = wd.get('emb_layer_norm_after.bias')
    x = O._ln(x, wd['emb_layer_norm_after.weight'].to(dtype), b.to(dtype) if b is not None else None)
    return O.lm_head(wd, x, dtype).cpu()


@pytest.mark.parametrize('kind,E,H', [('esm2', 1280, 20), ('esm2', 640, 20), ('esm2', 320, 20), ('esmc', 960, 15)])
def test_35000_residue_sequence(kind, E, H):
    """A 35 000-residue protein (titin) and a 3-residue neighbour, 2 layers, in 'fast', 'half' and 'exact': the fused rotary epilogue /
    qk_norm_rotary with tables grown past 32 768 rows and every attention form at S = 35 000, vs the oracle's math on the GPU; the
    neighbour (rotary positions 0 .. 2) bit-equal alone."""
    L, seed = 2, 31
    model = build(kind, L, E, H, seed)
    w = {k: v.bfloat16() for k, v in syn.synthetic_state_dict(kind, L, E, seed).items()}
    lengths = [35000, 3]
    tokens, cu = syn.random_tokens(lengths, seed=32), syn.cu_lens_of(lengths)
    ref32 = gpu_oracle_logits(w, H, tokens, cu, 35000, torch.float32)
    refbf = gpu_oracle_logits(w, H, tokens, cu, 35000, torch.bfloat16)
    torch.cuda.empty_cache()
    td, cd = tokens.to(DEV), cu.to(DEV)
    for mode in ('fast', 'half', 'exact'):
        model.set_precision(mode)
        what = f'{kind} E={E} H={H} (d={E // H}), 35 000 + 3 residues, precision {mode}'
        out = model(td, (cd, 35000))
        torch.cuda.synchronize()
        assert_parity(out, ref32, refbf, what)
        if mode != 'fast':
            assert rel_fro(out.float().cpu(), ref32) <= 1e-3, what
        alone = model(td[35000:], (syn.cu_lens_of([3]).to(DEV), 3))
        assert torch.equal(alone, out[35000:]), f'{what}: the 3-residue neighbour differs alone and packed'
    model.set_precision('fast')
