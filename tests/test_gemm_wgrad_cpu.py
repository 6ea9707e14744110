"""The weight-gradient GEMM without a GPU: the error bound of tests/gemm_wgrad_bounds.py accepts a float32 emulation of the kernel and
rejects every defect the emulation can switch on, on the shapes tests/test_gemm_wgrad_gpu.py runs; the host-side argument checks of
the entry points through the cross-compiled library; the bookkeeping of the new header (footprint coverage, binding table, exported
symbols, Makefile); the fixture of tests/test_full_train_gpu.py; and model.mark_trainable's flags on a CPU model."""
import ctypes
import os
import re

import pytest
import torch

import gemm_wgrad_bounds as WB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'esme_hip_gemm_wgrad.h')
CASES = [(M, nk) for M in WB.MS for nk in WB.NKS]
_SHARED = {}


def _case(M, nk):
    """Operands, the float64 reference and the bounds: computed once per shape, shared, never modified."""
    if (M, nk) not in _SHARED:
        N, K = nk
        dy, x, by, bx = WB.make_operands(M, N, K, seed=3 + M + N + K)
        _SHARED[M, nk] = dict(dy=dy, x=x, past=(by[M, 8:8 + N], bx[M, 8:8 + K]), ref=WB.reference_wgrad(dy, x),
                              bound={f: WB.wgrad_bound(dy, x, f) for f in WB.FMT})
    return _SHARED[M, nk]


@pytest.mark.parametrize('fmt', tuple(WB.FMT))
@pytest.mark.parametrize('M,nk', CASES)
def test_bound_accepts_the_correct_emulation(M, nk, fmt):
    c = _case(M, nk)
    worst = WB.worst(WB.emulate_wgrad(c['dy'], c['x'], fmt), c['ref'], c['bound'][fmt])
    print(f'M {M} (N, K) {nk} {fmt} correct emulation: worst err / bound {worst:.3f}')
    assert worst <= 1.0
    if M >= 63:                               # the bound resolves the signal: the largest gradient is far above the largest bound
        for r, b in zip(c['ref'], c['bound'][fmt]):
            assert float(r.abs().max()) >= 20 * float(b.max())


DEFECT_CASES = [(d, M, nk) for d in WB.DEFECTS for M, nk in CASES if WB.defect_applies(d, M, *nk)]


@pytest.mark.parametrize('defect,M,nk', DEFECT_CASES)
def test_bound_rejects_every_defect(defect, M, nk):
    """Every defect at every shape where it changes anything (gemm_wgrad_bounds.defect_applies says where it cannot: no tail at a
    multiple of 64 rows, no partials with one chunk, nothing but the row past M at M = 0); 'bf16_partials' is judged on fp32
    outputs, where the one output rounding cannot hide it."""
    c = _case(M, nk)
    for fmt in (('fp32',) if defect == 'bf16_partials' else tuple(WB.FMT)):
        worst = WB.worst(WB.emulate_wgrad(c['dy'], c['x'], fmt, defect, past=c['past']), c['ref'], c['bound'][fmt])
        print(f'M {M} (N, K) {nk} {fmt} {defect}: worst err / bound {worst:.1f}')
        assert worst > 1.0, f'the bound accepts the defect {defect!r}'


def test_every_defect_applies_somewhere_and_both_paths_occur():
    for d in WB.DEFECTS:
        assert any(WB.defect_applies(d, M, *nk) for M, nk in CASES), d
    chunks = {(M, nk): WB.split(M, *nk)[1] for M, nk in CASES}
    assert any(c == 1 for c in chunks.values()) and any(c > 1 for c in chunks.values())
    assert all(chunks[4099, nk] == 17 for nk in WB.NKS)
    assert WB.split(50000, 1280, 1280) == (10048, 5) and WB.split(50000, 5120, 1280) == (10048, 5) and WB.split(0, 64, 64) == (64, 1)
    assert WB.split(50000, 3840, 3840) == (50048, 1) and WB.split(70000, 64, 64) == (1152, 61) and WB.split(300, 64, 64) == (192, 2)


# ------------------------------------------------------------------ the header's bookkeeping

def _declared():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r'\b(esme_hip_\w+)\s*\(([^;{}]*?)\)\s*;', text)}


def test_every_pointer_entry_point_has_a_footprint_case():
    import test_gemm_wgrad_footprint_gpu as G
    names = [n for n, args in _declared().items() if '*' in args]
    assert names == ['esme_hip_gemm_wgrad']
    covered = {s for c in G.CASES for s in c.symbols}
    for n in names:
        assert n in covered, f'{n}: declared in esme_hip_gemm_wgrad.h with a pointer argument, but no case in tests/test_gemm_wgrad_footprint_gpu.py names it'
        assert re.search(rf'\b{n}\b', G.__doc__), f'{n}: missing from the docstring of tests/test_gemm_wgrad_footprint_gpu.py'
    assert covered <= set(_declared()), covered - set(_declared())
    ids = [c.id for c in G.CASES]
    assert len(ids) == len(set(ids))
    assert any('nodb' in i for i in ids) and any('nodb' not in i for i in ids)      # db present and NULL
    assert any('M65' in i for i in ids) and any('M4099' in i for i in ids) and any('bf16' in i for i in ids) and any('f32' in i for i in ids)


def test_header_symbols_exported_and_bound():
    from esme import _hip, _hip_gemm_wgrad
    declared = set(_declared())
    assert declared == set(_hip_gemm_wgrad.SIGNATURES) == {'esme_hip_gemm_wgrad_workspace_bytes', 'esme_hip_gemm_wgrad'}
    lib = ctypes.CDLL(_hip.lib_path())
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/esme_hip_gemm_wgrad.h but not exported'
    assert not declared & set(_hip.SIGNATURES)                                   # the main table and header keep their own symbols
    assert 'esme_hip_gemm_wgrad' not in open(os.path.join(ROOT, 'include', 'esme_hip.h')).read()
    for name, args in _declared().items():                                       # the number of arguments of each declaration equals the binding's
        assert len([a for a in args.split(',') if a.strip()]) == len(_hip_gemm_wgrad.SIGNATURES[name][1]), name
    mk = open(os.path.join(ROOT, 'esm-efficient_amd', 'csrc', 'Makefile')).read()
    assert 'gemm_wgrad.hip' in mk and 'esme_hip_gemm_wgrad.h' in mk


def test_host_validation_of_the_entry_points():
    """Host-side checks need no device: the size query's stated formula and geometry errors, and the argument errors that return
    before any launch."""
    from esme import _hip_gemm_wgrad as HW
    for M, nk in CASES + [(50000, (1280, 1280)), (50000, (5120, 1280)), (50000, (1280, 5120)), (50000, (3840, 1280)), (2 ** 31 - 1, (64, 64))]:
        assert HW.workspace_bytes(M, *nk) == WB.workspace_bytes(M, *nk), (M, nk)
    assert HW.workspace_bytes(50000, 1280, 1280) == 5 * (1280 * 1280 + 1280) * 4 and HW.workspace_bytes(200, 320, 192) == 0
    lib = HW._lib()
    q = lib.esme_hip_gemm_wgrad_workspace_bytes
    assert q(10, 33, 64) == -2 and b'multiples of 64' in lib.esme_hip_last_error()
    assert q(10, 64, 96) == -2 and q(-1, 64, 64) == -1 and q(2 ** 31, 64, 64) == -1 and q(10, 0, 64) == -1 and q(10, 64, -64) == -1
    with pytest.raises(RuntimeError, match='code -2'):
        HW.workspace_bytes(10, 33, 64)
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    need = HW.workspace_bytes(300, 64, 64)
    assert need == 2 * (64 * 64 + 64) * 4
    args = dict(dy=p, ld_dy=64, x=p, ld_x=64, M=300, N=64, K=64, dw=p, ld_dw=64, db=p, f32=0, ws=p, nb=need, stream=None)
    call = lambda **kw: lib.esme_hip_gemm_wgrad(*{**args, **kw}.values())
    for bad in (dict(dy=None), dict(x=None), dict(dw=None), dict(ws=None),                                         # null pointers
                dict(dy=p + 8), dict(x=p + 2), dict(dw=p + 4), dict(db=p + 8), dict(ws=p + 8),                     # misaligned
                dict(ld_dy=68), dict(ld_x=76), dict(ld_dw=66), dict(ld_dy=56), dict(ld_x=32), dict(ld_dw=0),        # strides
                dict(nb=need - 1), dict(nb=0), dict(M=-1), dict(M=2 ** 31), dict(N=0), dict(K=-64)):                # workspace, geometry
        assert call(**bad) == -1, bad
    assert call(nb=need - 1) == -1 and b'workspace too small' in lib.esme_hip_last_error()
    assert call(dy=p + 8) == -1 and b'misaligned' in lib.esme_hip_last_error()
    assert call(ld_x=76) == -1 and b'multiples of 8' in lib.esme_hip_last_error()
    assert call(N=33) == -2 and call(K=96) == -2 and b'multiples of 64' in lib.esme_hip_last_error()
    assert call(db=None, nb=need - 1) == -1                                          # (db = NULL is legal: the next refusal is the workspace's)


# ------------------------------------------------------------------ the fixture of tests/test_full_train_gpu.py

def test_full_grad_fixture_is_consistent():
    """g15_full_grad.npz / g15_full_grad_esmc.npz: every trained tensor of both models has its float16 truth, exponent and bar; the
    files hold data only and stay under the size limit; and the float64 oracle gradient of one tensor is reproduced here."""
    import numpy as np
    from golden_util import GOLDEN, load_golden
    from esme import synthetic as syn
    for name in ('g15_full_grad.npz', 'g15_full_grad_esmc.npz'):
        path = os.path.join(GOLDEN, name)
        assert os.path.getsize(path) < 1 << 20
        with np.load(path, allow_pickle=False) as z:
            assert all(z[k].dtype.kind in 'fiub' for k in z.files)
    g13 = load_golden('g13_lora.npz')
    g = {**load_golden('g15_full_grad.npz'), **load_golden('g15_full_grad_esmc.npz')}
    for kind in ('esm2', 'esmc'):
        L, E, seed = (int(g13[f'{kind}_{k}']) for k in ('L', 'E', 'seed'))
        want = {k for k in syn.synthetic_state_dict(kind, L, E, seed) if k.startswith('layers.') or k.startswith('emb_layer_norm_after.')}
        assert want == {k.split('/', 1)[1] for k in g if k.startswith(f'{kind}_oracle/') and not k.endswith('/loss')}
        for k in want:
            assert g[f'{kind}_oracle/{k}'].dtype == torch.float16 and 1.0 <= float(g[f'{kind}_oracle/{k}'].abs().max()) < 2.0
            assert 1e-3 < g[f'{kind}_bf16_error/{k}'] < 5e-2, (k, g[f'{kind}_bf16_error/{k}'])
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden_full_grad', os.path.join(GOLDEN, 'make_golden_full_grad.py'))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    src = open(os.path.join(GOLDEN, 'make_golden_full_grad.py')).read()
    assert 'import_reference' not in src and 'make_golden as' not in src          # the oracle only
    kind, name = 'esm2', 'layers.1.self_attn.out.weight'
    L, E, H, seed = (int(g13[f'{kind}_{k}']) for k in ('L', 'E', 'H', 'seed'))
    loss, grads = mk.step(syn.synthetic_state_dict(kind, L, E, seed), H, torch.float64, g[f'{kind}_tokens_in'], g[f'{kind}_tokens'],
                          g[f'{kind}_mask'], g['cu_lens'], int(g['max_len']))
    assert abs(float(loss) - g[f'{kind}_oracle/loss']) < 1e-9
    stored = g[f'{kind}_oracle/{name}'].double() * 2.0 ** int(g[f'{kind}_oracle_exp/{name}'])
    assert float((stored - grads[name]).norm() / grads[name].norm()) < 5e-4


# ------------------------------------------------------------------ mark_trainable on a CPU model

def _cpu_model(tmp_path, kind):
    from esme import ESM, synthetic as syn
    path = syn.write_checkpoint(str(tmp_path / f'{kind}.safetensors'), f'{kind}_t', 3, 64, 2, seed=5)
    return ESM.from_pretrained(path, device='cpu')


def _flags(model):
    return {n for n, p in model.named_parameters() if p.requires_grad}


@pytest.mark.parametrize('kind', ('esm2', 'esmc'))
def test_mark_trainable_flags(tmp_path, kind):
    model = _cpu_model(tmp_path, kind)
    keys = list(model.state_dict())
    assert _flags(model) == set()
    is_norm = lambda n: any(t in n for t in ('.norm.', '.layernorm_q.', '.layernorm_k.', '.final.0.'))
    proj = {n for n, _ in model.named_parameters() if n.startswith('layers.') and not is_norm(n)}
    norms = {n for n, _ in model.named_parameters() if n.startswith('layers.') and is_norm(n)}
    final_ln = {n for n, _ in model.named_parameters() if n.startswith('emb_layer_norm_after.')}
    assert proj and norms and final_ln and all(model.get_parameter(n).dim() == 1 for n in norms)
    assert model.mark_trainable() is model and _flags(model) == proj | norms | final_ln
    assert _flags(model.mark_trainable(norms=False)) == proj
    assert _flags(model.mark_trainable(projections=False)) == norms | final_ln
    only1 = {n for n in proj | norms if n.startswith('layers.1.')}
    assert _flags(model.mark_trainable(layers=[1])) == only1
    assert _flags(model.mark_trainable(layers=[-1, 0])) == {n for n in proj | norms if not n.startswith('layers.1.')}
    assert _flags(model.mark_trainable(False, False)) == set()
    with pytest.raises(IndexError):
        model.mark_trainable(layers=[3])
    # the LM head and the token embedding are not mark_trainable's: they keep their flags
    model.mark_lmhead(True).mark_trainable()
    assert {n for n in _flags(model) if n.startswith('lm_head.')} and 'embed_tokens.weight' not in _flags(model)
    model.mark_trainable(False, False)
    assert _flags(model) == {n for n, _ in model.named_parameters() if n.startswith('lm_head.')}
    assert list(model.state_dict()) == keys
    model.mark_lmhead(False).embed_tokens.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match='mark_trainable'):
        model.forward_trainable(torch.zeros(4, dtype=torch.long), (torch.tensor([0, 4], dtype=torch.int32), 4))


def test_mark_trainable_under_lora_and_routing_rule(tmp_path):
    """Under a LoRA wrapper the base `layer` is what mark_trainable selects; esme.autograd.frozen_linear sends a trainable projection
    to the kernels only when it is a layer's own and both widths are multiples of 64."""
    from esme import autograd as ag
    from esme.nn import Linear
    model = _cpu_model(tmp_path, 'esm2')
    model.add_lora(rank=4, alpha=8, adapter_names=['a'])
    lora = _flags(model)
    assert lora and all('.lora_' in n for n in lora)
    model.mark_trainable(norms=False, layers=[2])
    got = _flags(model) - lora
    assert got and all(n.startswith('layers.2.') for n in got) and any(n.endswith('self_attn.q.layer.weight') for n in got)
    seen = []
    orig = ag.TrainableLinear.apply
    try:
        ag.TrainableLinear.apply = staticmethod(lambda x, w, b, lin: seen.append(lin) or torch.nn.functional.linear(x, w, b))
        x = torch.zeros(3, 64, dtype=torch.bfloat16)
        lin = Linear(64, 128)
        lin.requires_grad_(True)
        ag.frozen_linear(x, lin)                                   # not a layer's own (the LM head's path): torch
        assert seen == []
        ag.frozen_linear(x, lin, True)
        assert seen == [lin]
        odd = Linear(64, 33)
        odd.requires_grad_(True)
        ag.frozen_linear(x, odd, True)                             # a width that is no multiple of 64: torch
        assert seen == [lin]
    finally:
        ag.TrainableLinear.apply = orig
