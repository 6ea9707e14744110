"""Every derived tensor -- the transformer block's weight copies, the padded embedding table and head weights, rotary tables, LoRA's stage
form -- is reported by esme.graph.external_tensors (no device: the builders are plain torch ops).

A captured hipGraph reads these copies through raw pointers and keeps alive only what external_tensors() lists, so a copy missing from it
can be freed under a live graph.  Each form the block can hand to a kernel -- plain, LayerNorm-folded, fp16, fp16 with an extension
K-tile, padded, LoRA -- is built here, looked up among the reported tensors by address, then rebuilt after a `p.data` edit +
invalidate_graphs(); the replaced tensors must no longer be reported."""
import pytest
import torch

from esme.esm import ESM2, ESMC
from esme.graph import external_tensors
from esme.nn import flatten_tensors

SEL = torch.tensor([3, 7, 64], dtype=torch.int32)          # a three-channel extension tile (HalfPlan.ext_sel)


def build(kind):
    torch.manual_seed(0)
    if kind == 'esm2':
        m = ESM2(num_layers=2, embed_dim=128, attention_heads=4)
    elif kind == 'esmc':
        m = ESMC(num_layers=2, embed_dim=128, attention_heads=2)
    else:
        m = ESM2(num_layers=2, embed_dim=120, attention_heads=5)        # head dim 24 -> 32, width 120 -> 128
        assert m.padded
    for p in m.parameters():
        p.data.normal_()
    return m.eval()


def weight_forms(model):
    """name -> callable returning one form of one layer's weights, for every form the model supports."""
    forms = {}
    for i, layer in enumerate(model.layers):
        att = layer.self_attn
        forms.update({
            f'{i} qkv plain': lambda att=att: att._weights_qkv(False),
            f'{i} out plain': lambda att=att: att._weights_out(),
            f'{i} up plain': lambda layer=layer: layer._weights_up(False),
            f'{i} down plain': lambda layer=layer: layer._weights_down(),
            f'{i} qkv folded': lambda att=att: att._weights_qkv(True),
            f'{i} up folded': lambda layer=layer: layer._weights_up(True),
            f'{i} qkv fp16': lambda att=att: (att._weights_qkv(True, True), att.stream_scale()),
            f'{i} up fp16': lambda layer=layer: (layer._weights_up(True, True), layer.stream_scale()),
            f'{i} out fp16': lambda att=att: att._weights_out(True),
            f'{i} down fp16': lambda layer=layer: layer._weights_down(True),
            f'{i} qkv fp16 ext': lambda att=att: att._weights_qkv(True, True, SEL),
            f'{i} up fp16 ext': lambda layer=layer: layer._weights_up(True, True, SEL),
        })
    return forms


def lora_forms(model):
    forms = {}
    for i, layer in enumerate(model.layers):
        for fold in (True, False):
            for names in (None, ['b']):
                forms[f'{i} lora fold={fold} names={names}'] = lambda att=layer.self_attn, fold=fold, names=names: att._lora_weights(names, fold)
    return forms


def reported(model):
    return {t.data_ptr() for t in external_tensors(model)}


def check_reported_and_rebuilt(model, forms):
    """Each form's tensors are reported right after it is built; after a `p.data` edit + invalidate_graphs() each form comes back in NEW tensors
    with other values, and none of the replaced ones (kept alive here, so no address is reused) is still reported."""
    old = {}
    for name, form in forms.items():
        tensors = list(flatten_tensors(form()))
        assert tensors, name
        missing = [tuple(t.shape) for t in tensors if t.data_ptr() not in reported(model)]
        assert not missing, f'{name}: tensors {missing} are not among external_tensors()'
        old[name] = tensors
    params = {p.data_ptr() for p in model.parameters()}
    derived = {n: [t for t in ts if t.data_ptr() not in params] for n, ts in old.items()}
    assert any(derived.values())
    before = {n: [t.clone() for t in ts] for n, ts in derived.items()}
    for p in model.parameters():
        p.data.mul_(1.25)
    model.invalidate_graphs()
    gone = {t.data_ptr() for ts in derived.values() for t in ts}
    for name, form in forms.items():
        tensors = list(flatten_tensors(form()))
        ptrs = {t.data_ptr() for t in tensors}
        assert ptrs <= reported(model), name
        assert not (ptrs & gone), f'{name}: a derived tensor survived the edit'
        fresh = [t for t in tensors if t.data_ptr() not in {p.data_ptr() for p in model.parameters()}]
        assert len(fresh) == len(before[name]), name
        if fresh:
            assert any(not torch.equal(a, b) for a, b in zip(fresh, before[name])), f'{name}: rebuilt with the old values'
    for form in forms.values():
        form()
    assert not (gone & reported(model)), 'a replaced derived tensor is still reported'


@pytest.mark.parametrize('kind', ('esm2', 'esmc', 'esm2_padded'))
def test_every_weight_form_is_reported_and_follows_an_edit(kind):
    model = build(kind)
    check_reported_and_rebuilt(model, weight_forms(model))


@pytest.mark.parametrize('kind', ('esm2', 'esmc'))
def test_lora_weight_forms_are_reported_and_follow_an_edit(kind):
    model = build(kind)
    model.add_lora(rank=8, alpha=8, layers=('query', 'value', 'output'), adapter_names=['a', 'b'])
    for p in model.parameters():
        p.data.normal_()                                  # (lora_B starts at zero)
    check_reported_and_rebuilt(model, lora_forms(model))
    check_reported_and_rebuilt(model, weight_forms(model))          # the base forms, read through the adapter wrappers


def test_padded_embedding_table_and_lm_head_are_reported_and_follow_an_edit():
    model = build('esm2_padded')
    check_reported_and_rebuilt(model, {'embed table': model._embed_table, 'lm head padded': model.lm_head._padded_weights})


def test_rotary_tables_of_every_dtype_are_reported_and_regrow_alone():
    model = build('esm2')
    rot = model.layers[0].self_attn.rot_emb
    pairs = {dt: rot.tables(90, 'cpu', dt) for dt in (torch.bfloat16, torch.float16, torch.float32)}
    ptrs = {dt: {t.data_ptr() for t in pair} for dt, pair in pairs.items()}
    assert all(p <= reported(model) for p in ptrs.values())          # all three at once
    cos, sin = rot.tables(410, 'cpu', torch.bfloat16)
    assert cos.shape[0] >= 410 and {cos.data_ptr(), sin.data_ptr()} <= reported(model)
    assert not (ptrs[torch.bfloat16] & reported(model)), 'the replaced bf16 pair is still reported'
    assert rot._cos_cached is cos and rot._sin_cached is sin
    for dt in (torch.float16, torch.float32):                       # untouched: same addresses, still reported
        assert {t.data_ptr() for t in rot.tables(90, 'cpu', dt)} == ptrs[dt] <= reported(model)
        assert rot._cos_cached.dtype == dt                          # the pair asked for last


def test_lora_stage_form_is_reported_and_follows_an_edit():
    model = build('esm2')
    model.add_lora(rank=8, alpha=8, layers=('query', 'value', 'output'), adapter_names=['a', 'b'])
    for p in model.parameters():
        p.data.normal_()
    q = model.layers[0].self_attn.q
    check_reported_and_rebuilt(model, {f'stage form names={names}': lambda names=names: q.stage_form(names) for names in (None, ['b'])})


def test_cls_head_padded_weight_is_reported_and_follows_an_in_place_write():
    from esme.head import ClsHead
    torch.manual_seed(0)
    head = ClsHead(120, num_cls=2, hidden_dim=64).eval()
    lin = head.head[0]
    w = head._mlp._weight(lin, 128)
    assert w.shape == (64, 128) and w.data_ptr() != lin.weight.data_ptr() and torch.equal(w[:, :120], lin.weight.data) and not w[:, 120:].any()
    assert w.data_ptr() in reported(head)
    assert head._mlp._weight(lin, 128) is w
    with torch.no_grad():
        lin.weight.copy_(torch.randn_like(lin.weight))
    w2 = head._mlp._weight(lin, 128)
    assert w2 is not w and torch.equal(w2[:, :120], lin.weight.data)
    assert w2.data_ptr() in reported(head) and w.data_ptr() not in reported(head)
