"""Adapters over a quantised base (QLoRA) without a GPU: the host-side argument checks of include/esme_hip_dequant_t.h through the
cross-compiled library, the header's bookkeeping (binding table, exported symbols, Makefile, footprint coverage), the definition of the
transposed layout restated in torch from the oracle's dequantisation (what tests/test_dequant_t_gpu.py compares the kernel with), and the
opt-in contract of add_lora(quantized_base=...) / forward_trainable on fixtures whose quantised state is set by hand: every refusal stays
in force until the model opted in, an opted-in model refuses a trainable LayerNorm by name, and once every check passes the first kernel
call says where it must run."""
import ctypes
import os
import re

import pytest
import torch

from oracle import esm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'esme_hip_dequant_t.h')
ENTRY_POINTS = ['esme_hip_dequantize_4bit_t', 'esme_hip_dequantize_8bit_t']
ARG, UNSUPPORTED = -1, -2
PAD = (torch.tensor([0, 4], dtype=torch.int32), 4)
TOK = torch.full((4,), 5, dtype=torch.long)


# ------------------------------------------------------------------ the header's bookkeeping

def _declared(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r'\b(esme_hip_\w+)\s*\(([^;{}]*?)\)\s*;', text)}


def test_header_symbols_exported_and_bound():
    from esme import (_hip, _hip_attn_bwd, _hip_attn_maps, _hip_attn_pool_bwd, _hip_contact_features, _hip_contacts, _hip_dequant_t,
                      _hip_gemm_wgrad, _hip_optim)
    declared = _declared()
    assert list(declared) == list(_hip_dequant_t.SIGNATURES) == ENTRY_POINTS
    lib = ctypes.CDLL(_hip.lib_path())
    for name, args in declared.items():
        assert hasattr(lib, name), f'{name} declared in include/esme_hip_dequant_t.h but not exported'
        assert len([a for a in args.split(',') if a.strip()]) == len(_hip_dequant_t.SIGNATURES[name][1]), name
    for other in (_hip, _hip_attn_bwd, _hip_attn_maps, _hip_attn_pool_bwd, _hip_contact_features, _hip_contacts, _hip_gemm_wgrad, _hip_optim):
        assert not set(declared) & set(other.SIGNATURES), other.__name__
    for other in os.listdir(os.path.join(ROOT, 'include')):
        if other != 'esme_hip_dequant_t.h':
            assert not set(declared) & set(_declared(os.path.join(ROOT, 'include', other))), other
    mk = open(os.path.join(ROOT, 'esm-efficient_amd', 'csrc', 'Makefile')).read()
    assert 'quant_t.hip' in mk and 'esme_hip_dequant_t.h' in mk


def test_every_pointer_entry_point_has_a_footprint_case():
    import test_dequant_t_footprint_gpu as G
    names = [n for n, args in _declared().items() if '*' in args]
    assert names == ENTRY_POINTS
    covered = {s for c in G.CASES for s in c.symbols}
    for n in names:
        assert n in covered, f'{n}: no case in tests/test_dequant_t_footprint_gpu.py names it'
        assert re.search(rf'\b{n}\b', G.__doc__), f'{n}: missing from the docstring of tests/test_dequant_t_footprint_gpu.py'
    assert covered <= set(_declared())
    ids = [c.id for c in G.CASES]
    assert len(ids) == len(set(ids))


# ------------------------------------------------------------------ host validation: every refusal returns before any launch

def test_host_validation_of_the_entry_points():
    from esme import _hip_dequant_t as HT
    from esme.quantization import FP4_CODEBOOK
    lib = HT._lib()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    cb = (ctypes.c_float * 16)(*FP4_CODEBOOK)
    err = lib.esme_hip_last_error

    def c4(**kw):
        a = dict(codes=p, absmax=p, N=16, K=64, cb=cb, out=p, ldo=16, stream=None)
        a.update(kw)
        return lib.esme_hip_dequantize_4bit_t(*a.values())

    def c8(**kw):
        a = dict(codes=p, scale=p, N=16, K=64, out=p, ldo=16, stream=None)
        a.update(kw)
        return lib.esme_hip_dequantize_8bit_t(*a.values())

    for call, name in ((c4, b'dequantize_4bit_t'), (c8, b'dequantize_8bit_t')):
        assert call(N=-1) == ARG and b'bad sizes' in err() and name in err()
        assert call(K=0) == ARG and call(K=-64) == ARG
        assert call(N=0) == 0 and call(N=0, codes=None, out=None, ldo=0) == 0                 # nothing to write: no launch, no pointer needed
        assert call(ldo=8) == ARG and b'bad stride' in err()                                  # ldo < N
        assert call(ldo=20) == ARG and b'misaligned' in err()                                 # ldo % 8
        assert call(N=9, ldo=12) == ARG
        assert call(out=p + 2) == ARG and b'misaligned' in err() and call(out=p + 8) == ARG   # out: 16 bytes
        assert call(codes=None) == ARG and b'null' in err() and call(out=None) == ARG
        assert call(**{'absmax' if call is c4 else 'scale': None}) == ARG
    # 4-bit: blocks of 64, 4-byte code words, a codebook of 16 host floats in [-1, 1]
    for K in (8, 32, 72, 96):
        assert c4(K=K) == UNSUPPORTED and b'multiple of the block size 64' in err()
    assert c4(codes=p + 1) == ARG and c4(codes=p + 2) == ARG and b'misaligned' in err()
    assert c4(cb=None) == ARG and b'codebook' in err()
    for bad in (1.5, -1.0001, float('nan'), float('inf')):
        vals = list(FP4_CODEBOOK)
        vals[9] = bad
        assert c4(cb=(ctypes.c_float * 16)(*vals)) == ARG and b'codebook' in err(), bad
    # int8: K a multiple of 8, 8-byte code words
    for K in (4, 12, 63):
        assert c8(K=K) == UNSUPPORTED and b'multiple of 8' in err()
    assert c8(codes=p + 4) == ARG and b'misaligned' in err() and c8(codes=p + 1) == ARG
    # the wrappers refuse CPU tensors, as every wrapper of the package does
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        HT.dequantize_4bit_t(torch.zeros(1, 32, dtype=torch.uint8), torch.zeros(1, 1), FP4_CODEBOOK)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        HT.dequantize_8bit_t(torch.zeros(1, 8, dtype=torch.int8), torch.zeros(1))


# ------------------------------------------------------------------ the definition of the transposed layout

def transposed_4bit(codes, absmax, codebook, ldo=None):
    """out (K, ldo) bf16 with out[k, n] = bf16(codebook[code(n, k)] * absmax[n, k // 64]) for n < N, written index by index over the
    TRANSPOSED index space (element 2 i of a row in the high nibble of byte i); columns N .. ldo - 1 stay zero here (untouched there)."""
    N, K = codes.shape[0], codes.shape[1] * 2
    out = torch.zeros(K, ldo or N, dtype=torch.bfloat16)
    cb = torch.tensor(codebook, dtype=torch.float32)
    k, n = torch.meshgrid(torch.arange(K), torch.arange(N), indexing='ij')
    byte = codes[n, k // 2].to(torch.int64)
    idx = torch.where(k % 2 == 0, byte >> 4, byte & 15)
    out[:, :N] = (cb[idx] * absmax[n, k // O.QUANT_BLOCK]).to(torch.bfloat16)
    return out


def transposed_8bit(codes, scale, ldo=None):
    N, K = codes.shape
    out = torch.zeros(K, ldo or N, dtype=torch.bfloat16)
    k, n = torch.meshgrid(torch.arange(K), torch.arange(N), indexing='ij')
    out[:, :N] = (codes[n, k].float() * scale.float()[n] / 127.).to(torch.bfloat16)
    return out


@pytest.mark.parametrize('N,K', [(1, 64), (65, 128), (129, 320)])
def test_transposed_layout_is_the_transpose_of_the_oracle_expansion(N, K):
    """What tests/test_dequant_t_gpu.py holds the kernel to, dequantize(...).t().contiguous(), element by element."""
    from esme.quantization import CODEBOOKS
    g = torch.Generator().manual_seed(N)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
    for cb in CODEBOOKS.values():
        codes, absmax = O.quantize_4bit(w, cb)
        absmax[0, 0] = 0.0
        want = O.dequantize_4bit(codes, absmax, cb).t().contiguous()
        assert torch.equal(transposed_4bit(codes, absmax, cb), want) and not bool(want[:64, 0].any())
        wide = transposed_4bit(codes, absmax, cb, ldo=N + 24)
        assert torch.equal(wide[:, :N], want) and not bool(wide[:, N:].any())
    codes, scale = O.quantize_8bit(w)
    assert torch.equal(transposed_8bit(codes, scale), O.dequantize_8bit(codes, scale).t().contiguous())


# ------------------------------------------------------------------ the opt-in contract, on fixtures with hand-set quantised state

def _model(kind='esm2', **kw):
    from esme import ESM2, ESMC
    cls, heads = (ESM2, 4) if kind == 'esm2' else (ESMC, 2)
    return cls(**{'num_layers': 1, 'embed_dim': 128, 'attention_heads': heads, **kw})


def _quantised(kind='esm2'):
    """A one-layer model whose projections are Linear4bit modules over the oracle's codes, with the markers quantize_model_ leaves
    (the packed matrices of the fused forward need a device: placeholders stand in for them)."""
    from esme.quantization import Linear4bit, WeightScratch
    m = _model(kind)
    scratch = WeightScratch()

    def q(lin):
        w = torch.nan_to_num(lin.weight.data.float()).clamp(-1, 1).to(torch.bfloat16)
        mod = Linear4bit(*O.quantize_4bit(w), lin.bias.data if lin.bias is not None else None)
        mod.scratch = scratch
        return mod
    layer = m.layers[0]
    att = layer.self_attn
    for p in ('q', 'k', 'v', 'out'):
        setattr(att, p, q(getattr(att, p)))
    if kind == 'esm2':
        layer.final[1], layer.final[3] = q(layer.final[1]), q(layer.final[3])
    else:
        sw = layer.final[1]
        sw.activation, sw.fc, layer.final[2] = q(sw.activation), q(sw.fc), q(layer.final[2])
    att._q4_qkv = att._q4_out = layer._q4_up = layer._q4_down = object()
    m.quantization, m._q4_scratch = '4bit-fp4', scratch
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def test_add_lora_keeps_refusing_a_quantised_model_without_the_keyword():
    for m in (_quantised(), _model()):
        m.quantization = '4bit'
        for kw in ({}, {'quantized_base': False}):
            with pytest.raises(NotImplementedError, match='quanti') as e:
                m.add_lora(rank=4, alpha=4, **kw)
            assert 'quantization= is not supported with adapters' in str(e.value) and 'quantized_base=True' in str(e.value)
        assert not m.has_lora
    # hand-set markers on a model that never opted in: the inference path of the adapters and forward_trainable refuse as before
    m = _model().add_lora(rank=4, alpha=4)
    att = m.layers[0].self_attn
    att._q4_qkv = object()
    with pytest.raises(NotImplementedError, match='need unquantised bfloat16 base weights') as e:
        att._lora_weights(None, True)
    assert 'quantized_base=True' in str(e.value)
    for mode in (m.train, m.eval):
        mode()
        with pytest.raises(NotImplementedError, match='quantised') as e:
            m.forward_trainable(TOK, PAD)
        assert 'quantized_base=True' in str(e.value)
    att._q4_qkv = None
    m.layers[0]._q4_down = object()
    with pytest.raises(NotImplementedError, match='quantised'):
        m.forward_trainable(TOK, PAD)
    m.layers[0]._q4_down = None
    m.quantization = '8bit'
    with pytest.raises(NotImplementedError, match='quantised'):
        m.forward_trainable(TOK, PAD)


def test_quantized_base_on_an_unquantised_model_is_a_plain_add_lora():
    from esme.lora import LoRA
    from esme.nn import Linear
    torch.manual_seed(0)
    a = _model().add_lora(rank=4, alpha=8, quantized_base=True)
    torch.manual_seed(0)
    b = _model().add_lora(rank=4, alpha=8)
    assert list(a.state_dict()) == list(b.state_dict()) and a.lora_kwargs == b.lora_kwargs
    assert [n for n, p in a.named_parameters() if p.requires_grad] == [n for n, p in b.named_parameters() if p.requires_grad]
    att = a.layers[0].self_attn
    assert isinstance(att.q, LoRA) and type(att.q.layer) is Linear and not isinstance(att.k, LoRA)
    assert a.has_lora and not a._qlora and not att._qlora and not a.layers[0]._qlora
    a.quantization = '4bit'                                   # it did not opt in to anything: the refusals hold
    with pytest.raises(NotImplementedError, match='quantised'):
        a.forward_trainable(TOK, PAD)


@pytest.mark.parametrize('kind', ('esm2', 'esmc'))
def test_an_opted_in_model_refuses_what_it_cannot_train_and_then_reaches_the_kernels(kind):
    from esme.lora import LoRA
    from esme.quantization import Linear4bit
    m = _quantised(kind)
    with pytest.raises(NotImplementedError, match='quantised'):           # quantised, not opted in
        m.forward_trainable(TOK, PAD)
    assert m.add_lora(rank=4, alpha=4, quantized_base=True) is m
    layer = m.layers[0]
    att = layer.self_attn
    assert m._qlora and att._qlora and layer._qlora and m.has_lora
    assert isinstance(att.q, LoRA) and isinstance(att.q.layer, Linear4bit) and att.q.lora_A['default'].dtype == torch.bfloat16
    trainable = [n for n, p in m.named_parameters() if p.requires_grad]
    assert trainable and all('.lora_' in n for n in trainable)
    assert not att.q.layer.weight.requires_grad and att.q.layer.weight.dtype == torch.uint8
    # the codes are not trainable
    with pytest.raises(NotImplementedError, match='stored quantised'):
        m.mark_trainable()
    # a LayerNorm that requires grad is refused by name
    norms = [('layers.0.self_attn.norm.weight', att.norm.weight, 'self_attn.norm.weight'), ('final.0', layer.final[0].weight, r'final\.0\.weight'),
             ('emb_layer_norm_after', m.emb_layer_norm_after.weight, r'emb_layer_norm_after\.weight')]
    if layer.final[0].bias is not None:
        norms.append(('final.0 bias', layer.final[0].bias, r'final\.0\.bias'))
    if kind == 'esmc':
        norms.append(('layernorm_q', att.layernorm_q.weight, r'self_attn\.layernorm_q\.weight'))
    for _, p, pat in norms:
        p.requires_grad_(True)
        for mode in (m.train, m.eval):
            mode()
            with pytest.raises(NotImplementedError, match=pat) as e:
                m.forward_trainable(TOK, PAD)
            assert 'quantised base' in str(e.value)
        p.requires_grad_(False)
    # the unchanged refusals
    m.precision = 'high'
    with pytest.raises(NotImplementedError, match='precision'):
        m.forward_trainable(TOK, PAD)
    m.precision = 'fast'
    with pytest.raises(NotImplementedError, match='LoRA'):
        m.graphed(TOK, PAD)
    with pytest.raises(NotImplementedError, match='unquantised bfloat16'):
        att.q(torch.zeros(2, 128, dtype=torch.bfloat16))           # the stand-alone LoRA.forward
    # the LM head may train; every check passed: the first kernel call says where it must run
    m.mark_lmhead(True)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.forward_trainable(TOK, PAD)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        layer.forward_trainable(torch.zeros(4, 128, dtype=torch.bfloat16), *PAD)
