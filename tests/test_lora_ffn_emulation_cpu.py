"""The FFN-adapter path restated on the CPU from the derived weights the layer builds (FlashTransformerLayer._ffn_lora_weights), against
the float64 statement of the reference's data flow -- the comparison tests/test_lora_ffn_gpu.py makes on the device (its item 3), here
in fp32 / bf16 torch ops with the kernels' rounding points.  Two things follow without a device:

 * the derived weights are right: the stacked A' with c1A / bA, the extension columns in SwiGLU's interleaved rows and the extended
   down weight reproduce  LayerNorm -> up + adapters -> GELU / silu(g) f -> down + adapters  as closely as the adapter-free forms
   reproduce the adapter-free branch;
 * the bar of that comparison (relative Frobenius error at most max(1.25 x the adapter-free error, 4e-3)) rejects the defects a
   review would look for: the scaling alpha / rank dropped, the gate adapter's columns applied to the fc rows (and the reverse), and
   the extension read one column off."""
import pytest
import torch
import torch.nn.functional as F

from esme import ESM, synthetic as syn
from esme.lora import LoRA
from golden_util import rel_fro

L, E, H, T = 2, 128, 2, 96
ALL_SIX = ('query', 'key', 'value', 'output', 'ffn_up', 'ffn_down')
SCALING = 1.5


def _bf(t):
    return t.to(torch.bfloat16)


def model_of(kind, tmp_path, adapters):
    path = syn.write_checkpoint(str(tmp_path / f'{kind}.safetensors'), f'{kind}_t', L, E, H, seed=9)
    model = ESM.from_pretrained(path, device='cpu')
    if adapters:
        torch.manual_seed(3)
        model.add_lora(rank=16, alpha=24, layers=ALL_SIX, adapter_names=['a', 'b'])
        gen = torch.Generator().manual_seed(1)
        with torch.no_grad():
            for k, p in sorted(model.named_parameters()):
                if '.lora_B.' in k:
                    p.copy_((torch.randn(p.shape, generator=gen) * 0.1 / p.shape[1] ** 0.5).to(p.dtype))
    return model


def stream(seed=0):
    g = torch.Generator().manual_seed(seed)
    return _bf(torch.randn(T, E, generator=g) * (0.5 + torch.rand(1, E, generator=g)) + 0.25)


@torch.no_grad()
def branch64(layer, x, adapters=True):
    ln = layer.final[0]
    h = F.layer_norm(x.double(), (E,), ln.weight.double(), ln.bias.double() if ln.bias is not None else None, ln.eps)

    def lin(m, v):
        base = m.layer if isinstance(m, LoRA) else m
        y = F.linear(v, base.weight.double(), base.bias.double() if base.bias is not None else None)
        if adapters and isinstance(m, LoRA):
            for n in m.select(None):
                y = y + F.linear(F.linear(v, m.lora_A[n].double()), m.lora_B[n].double()) * m.scaling
        return y
    ups, (_, down) = layer._ffn_projections()
    u = F.gelu(lin(ups[0][1], h)) if len(ups) == 1 else F.silu(lin(ups[0][1], h)) * lin(ups[1][1], h)
    return lin(down, u) / layer.residue_scaling


@torch.no_grad()
def emulate(layer, x, defect=None):
    """FlashTransformerLayer._ffn / _ffn_lora, LayerNorm-folded, onto a zero residual: fp32 statistics and epilogues, exact products
    summed in float64 and rounded to fp32 (the MFMA chain's fp32 accumulator), bf16 where a kernel writes bf16."""
    ln, gelu = layer.final[0], layer.final_activation == 'gelu'
    ups, (_, down) = layer._ffn_projections()
    FF = ups[0][1].out_features
    lw = layer._ffn_lora_weights(None, True) if layer._has_lora else {'up': None, 'down': None}
    x32 = x.float()
    mean = x32.mean(1, keepdim=True)
    var = ((x32 * x32).mean(1, keepdim=True) - mean * mean).clamp_min(0.0) + ln.eps
    rstd, sd = var.rsqrt(), var.sqrt()
    w, c1, c2 = layer._pack_fold()
    xe = x

    def broken(we, K, rows_interleaved):
        ext = we[:, K:].clone()
        if defect == 'no_scaling':
            ext = _bf(ext.float() / SCALING)
        elif defect == 'offset':
            ext = torch.roll(ext, 1, dims=1)
        elif defect == 'gate_fc_swapped' and rows_interleaved:
            ext = ext.view(FF // 32, 2, 32, -1).flip(1).reshape(2 * FF, -1)
        return torch.cat((we[:, :K], ext), 1)
    if lw['up'] is not None:
        X, A, c1A, bA, we = lw['up']
        u = _bf(sd * bA + ((x.double() @ A.double().T).float() - mean * c1A))
        xe = torch.cat((x, u, torch.zeros(T, X - u.shape[1], dtype=torch.bfloat16)), 1)
        w = broken(we, E, not gelu)
    y = rstd * (xe.double() @ w.double().T).float() + (c2 - (rstd * mean) * c1)
    if gelu:
        act = _bf(F.gelu(y))
    else:
        y = y.view(T, FF // 32, 2, 32)
        act = _bf(F.silu(y[:, :, 0]) * y[:, :, 1]).reshape(T, FF)
    wd, bd = (down.layer if isinstance(down, LoRA) else down).weight.data, down.bias
    if lw['down'] is not None:
        X, A, we = lw['down']
        u = _bf((act.double() @ A.double().T).float())
        act = torch.cat((act, u, torch.zeros(T, X - u.shape[1], dtype=torch.bfloat16)), 1)
        wd = broken(we, FF, False)
    acc = (act.double() @ wd.double().T).float()
    if bd is not None:
        acc = acc + bd.float()
    return _bf(acc / layer.residue_scaling)


def bar_of(kind, tmp_path, x):
    base = model_of(kind, tmp_path, False).layers[0]
    e_base = rel_fro(emulate(base, x).double(), branch64(base, x))
    return max(1.25 * e_base, 4e-3), e_base


@pytest.mark.parametrize('kind', ['esm2', 'esmc'])
def test_derived_weights_reproduce_the_float64_branch(kind, tmp_path):
    x = stream()
    bar, e_base = bar_of(kind, tmp_path, x)
    layer = model_of(kind, tmp_path, True).layers[0]
    assert layer.final[1 if kind == 'esm2' else 2].scaling == SCALING
    ref = branch64(layer, x)
    e = rel_fro(emulate(layer, x).double(), ref)
    share = rel_fro(ref, branch64(layer, x, adapters=False))
    print(f'\n[lora-ffn emulation] {kind}: adapter-free {e_base:.3e} | all FFN adapters {e:.3e} | bar {bar:.3e} | adapters move the branch by {share:.2f} of its norm')
    assert share > 0.05 and e <= bar
    assert e_base > 1e-3, 'an emulation without the bf16 roundings would make the bar meaningless'


@pytest.mark.parametrize('kind,defect', [('esm2', 'no_scaling'), ('esm2', 'offset'), ('esmc', 'no_scaling'), ('esmc', 'offset'), ('esmc', 'gate_fc_swapped')])
def test_the_bar_rejects_defects(kind, defect, tmp_path):
    x = stream(1)
    bar, _ = bar_of(kind, tmp_path, x)
    layer = model_of(kind, tmp_path, True).layers[0]
    ref = branch64(layer, x)
    assert rel_fro(emulate(layer, x).double(), ref) <= bar
    e = rel_fro(emulate(layer, x, defect).double(), ref)
    print(f'\n[lora-ffn emulation] {kind} {defect}: {e:.3e} against the bar {bar:.3e}')
    assert e > bar, defect
