#!/usr/bin/env python
"""Generate the golden fixtures in this directory from the REFERENCE itself.

Runs only in the authoring container (needs /root/reference; never on the GPU
box).  It imports the reference package `esme` from /root/reference with a
pure-torch stand-in for the three third-party `flash_attn` symbols the
reference imports (the wheel is not installable offline), builds reference
models from this project's deterministic synthetic checkpoints
(`esme.synthetic`, numpy PCG64 -- regenerated from a seed on every box, so only
inputs + expected outputs are stored), runs them on CPU in fp32 and in the
reference's default bf16, and writes small .npz files.

    python tests/golden/make_golden.py            # rewrites tests/golden/*.npz

Nothing of the reference's source is copied: the fixtures are data (inputs and
the reference's outputs).  The stand-in below is this project's own code and
is the *specification* used at the flash_attn seam.
"""
import importlib.util
import json
import math
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
from golden_util import exact_cpu_gemms      # noqa: E402  (bf16 fields: GEMMs rounded once, the same on every CPU)
REF = '/root/reference'


# ----------------------------------------------------------------- stand-in
def _flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q,
                            max_seqlen_k, dropout_p=0.0, softmax_scale=None,
                            causal=False, **_):
    assert not causal and dropout_p == 0.0
    scale = softmax_scale or 1.0 / math.sqrt(q.shape[-1])
    out = torch.empty_like(q)
    cu = cu_seqlens_q.tolist()
    for a, b in zip(cu[:-1], cu[1:]):
        qs, ks, vs = (t[a:b].float().transpose(0, 1) for t in (q, k, v))
        p = torch.softmax(qs @ ks.transpose(1, 2) * scale, dim=-1)
        out[a:b] = (p @ vs).transpose(0, 1).to(q.dtype)
    return out


def _unpad_input(hidden_states, attention_mask, unused_mask=None):
    lens = attention_mask.sum(dim=-1, dtype=torch.int32)
    idx = torch.nonzero(attention_mask.flatten(), as_tuple=False).flatten()
    cu = torch.nn.functional.pad(torch.cumsum(lens, 0, dtype=torch.int32), (1, 0))
    flat = hidden_states.reshape(-1, *hidden_states.shape[2:])
    return flat[idx], idx, cu, int(lens.max()), lens


def _pad_input(hidden_states, indices, batch, seqlen):
    out = torch.zeros(batch * seqlen, *hidden_states.shape[1:],
                      dtype=hidden_states.dtype, device=hidden_states.device)
    out[indices] = hidden_states
    return out.view(batch, seqlen, *hidden_states.shape[1:])


def import_reference():
    fa = types.ModuleType('flash_attn')
    fa.flash_attn_varlen_func = _flash_attn_varlen_func
    bp = types.ModuleType('flash_attn.bert_padding')
    bp.pad_input, bp.unpad_input = _pad_input, _unpad_input
    fa.bert_padding = bp
    sys.modules['flash_attn'] = fa
    sys.modules['flash_attn.bert_padding'] = bp
    sys.path.insert(0, REF)
    import esme as ref            # noqa: E402  (the reference package)
    assert ref.__file__.startswith(REF), ref.__file__
    return ref


def load_synthetic():
    """Load this project's esme/synthetic.py by path (the name `esme` is taken
    by the reference package inside this process)."""
    spec = importlib.util.spec_from_file_location(
        'amd_synthetic', os.path.join(ROOT, 'esm-efficient_amd', 'esme', 'synthetic.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bits(t):
    """bf16 tensor -> uint16 numpy (exact)."""
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16)


def f32(t):
    """fp32 outputs as float32; bf16 outputs as their exact uint16 bit patterns
    (tests/golden_util.py `load_golden` converts them back)."""
    if t.dtype == torch.bfloat16:
        return bits(t)
    return t.detach().float().numpy()


# ------------------------------------------------------------------ helpers
def build_ref_model(ref, syn, kind, L, E, H, seed, dtype):
    cls = ref.ESM2 if kind == 'esm2' else ref.ESMC
    model = cls(num_layers=L, embed_dim=E, attention_heads=H, dtype=dtype)
    sd = syn.synthetic_state_dict(kind, L, E, seed)
    missing, unexpected = model.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=True)
    assert not missing and not unexpected
    return model.eval()


def layer_taps(model, x, cu_lens, max_len, layer_idx=0):
    """Stage taps of one reference layer, produced by calling the reference's
    own sub-modules in the order FlashTransformerLayer.forward does."""
    layer = model.layers[layer_idx]
    att = layer.self_attn
    T, E = x.shape
    taps = {}
    h = att.norm(x)
    q, k, v = att._qkv(x)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    qr, kr = att.rot_emb(q, k, cu_lens, max_len)
    a = att._attn(qr, kr, v, cu_lens, max_len)
    o = att.out(a)
    x1 = x + o / layer.residue_scaling
    h2 = layer.final[0](x1)
    mid = layer.final[1](h2)
    if len(layer.final) == 4:
        mid = layer.final[2](mid)
        y = layer.final[3](mid)
    else:
        y = layer.final[2](mid)
    x2 = x1 + y / layer.residue_scaling
    full = layer(x, cu_lens, max_len)
    assert torch.equal(full, x2)
    taps.update(ln1=h, q=q.reshape(T, E), k=k.reshape(T, E), v=v.reshape(T, E),
                q_rot=qr.reshape(T, E), k_rot=kr.reshape(T, E), attn=a, attn_out=o,
                x_attn=x1, ln2=h2, ffn_mid=mid, ffn_out=y, x_out=x2)
    return taps


def main():
    torch.set_grad_enabled(False)
    torch.manual_seed(0)
    ref = import_reference()
    syn = load_synthetic()
    from esme.alphabet import tokenize, tokenize_unpad, Alphabet, Alphabet3
    from esme.rotary import RotaryEmbedding, culen_indices
    out = {}

    # ---- G6 tokenizer known answers --------------------------------------
    p53 = ('MEEPQSDPSVEPPLSQETFSDLWKLLPENNVLSPLPSQAMDDLMLSPDDIEQWFTEDPGPDEAPRMPEAAPPVAPAPAAPTPAAPAPAPSWPLSSSVPSQKTYQGSYGFRLGFLHSGTAKSVTCTYSPALNKMFCQLAKTCPVQLWVDSTPPPGTRVRAMAIYKQSQHMTEVVRRCPHHERCSDSDGLAPPQHLIRVEGNLRVEYLDDRNTFRHSVVVPYEPPEVGSDCTTIHYNYMCNSSCMGGMNRRPILTIITLEDSSGNLLGRNSFEVRVCACPGRDRRTEEENLRKKGEPHHELPPGSTKRALPNNTSSSPQPKKKPLDGEYFTLQIRGRERFEMFRELNEALELKDAQAGKEPGGSRAHSSHLKSKKGQSTSRHKKLMFKTEGPDSD')
    readme = ['MEEPQSDPSVEPPLSQESTFSLDLWK', 'MADQLTEEQIAEFKEAFSLFDKDG']
    odd = ['MK<mask>LVJ*', 'ACDEFGHIKLMNPQRSTVWYXBUZO.-', 'M']
    tok = {}
    for name, seqs in (('p53', [p53]), ('readme', readme), ('odd', odd), ('p53x2', [p53, p53 + p53])):
        for aname, alpha in (('esm2', Alphabet), ('esmc', Alphabet3)):
            padded = tokenize(seqs, alphabet=alpha)
            t, idx, cu, ml = tokenize_unpad(seqs, alphabet=alpha)
            tok[f'{name}/{aname}'] = dict(seqs=seqs, padded=padded.tolist(), packed=t.tolist(),
                                          indices=idx.tolist(), cu_lens=cu.tolist(), max_len=int(ml))
    with open(os.path.join(HERE, 'g6_tokenizer.json'), 'w') as f:
        json.dump(tok, f)

    # ---- G5 rotary tables + positions -------------------------------------
    cu5 = torch.tensor([0, 60, 100, 280], dtype=torch.int32)
    g5 = {'cu_lens': cu5.numpy(), 'positions': culen_indices(cu5).numpy()}
    for d in (16, 32, 64):
        for dt, tag in ((torch.float32, 'f32'), (torch.bfloat16, 'bf16')):
            rot = RotaryEmbedding(dim=d)
            rot._update_cos_sin_cache(180, device=torch.device('cpu'), dtype=dt)
            g5[f'cos_d{d}_{tag}'] = f32(rot._cos_cached)
            g5[f'sin_d{d}_{tag}'] = f32(rot._sin_cached)
    # rotary applied to a seeded tensor (fp32 and bf16)
    rng = np.random.Generator(np.random.PCG64(5))
    xq = torch.from_numpy(rng.standard_normal((280, 4, 32), dtype=np.float32))
    xk = torch.from_numpy(rng.standard_normal((280, 4, 32), dtype=np.float32))
    for dt, tag in ((torch.float32, 'f32'), (torch.bfloat16, 'bf16')):
        rot = RotaryEmbedding(dim=32)
        qr, kr = rot(xq.to(dt), xk.to(dt), cu5, 180)
        g5[f'q_rot_{tag}'], g5[f'k_rot_{tag}'] = f32(qr), f32(kr)
    g5['q_in'], g5['k_in'] = xq.numpy(), xk.numpy()
    np.savez_compressed(os.path.join(HERE, 'g5_rotary.npz'), **g5)

    # ---- G1 tiny ESM2: full forward + per-stage taps -----------------------
    def run_model_fixture(fname, kind, L, E, H, seed, lengths, mask_at=(), tap_rows=None,
                          store_taps=True, with_padded=False, layers_arg=None):
        g = {'kind': kind, 'L': L, 'E': E, 'H': H, 'seed': seed}
        tokens = syn.random_tokens(lengths, seed=seed)
        for m in mask_at:
            tokens[m] = 32
        cu = syn.cu_lens_of(lengths)
        max_len = max(lengths)
        g.update(tokens=tokens.numpy(), cu_lens=cu.numpy(), max_len=max_len)
        rows = np.arange(tokens.numel()) if tap_rows is None else np.asarray(tap_rows)
        g['tap_rows'] = rows
        for dt, tag in ((torch.float32, 'f32'), (torch.bfloat16, 'bf16')):
            with exact_cpu_gemms(dt == torch.bfloat16):
                model = build_ref_model(ref, syn, kind, L, E, H, seed, dt)
                logits = model(tokens, (cu, max_len))
                g[f'logits_{tag}'] = f32(logits)
                g[f'logprob_{tag}'] = f32(model.predict_log_prob(tokens, (cu, max_len)))
                rep = model.forward_representation(tokens, (cu, max_len))
                g[f'rep_{tag}'] = f32(rep)[rows]
                if layers_arg is not None:
                    g['layers_arg'] = np.asarray(layers_arg)
                    g[f'rep_layers_{tag}'] = f32(model.forward_representation(
                        tokens, (cu, max_len), layers=list(layers_arg)))[rows]
                if store_taps:
                    x0 = model.embedding(tokens) if kind == 'esm2' else model.embed_tokens(tokens)
                    g[f'emb_{tag}'] = f32(x0)[rows]
                    for name, t in layer_taps(model, x0, cu, max_len, 0).items():
                        g[f'l0_{name}_{tag}'] = f32(t)[rows]
                if with_padded:
                    # 2-D path: pad the same sequences to (B, max_len)
                    B = len(lengths)
                    tok2d = torch.full((B, max_len), 1, dtype=torch.int64)
                    for i, (a, b) in enumerate(zip(cu[:-1].tolist(), cu[1:].tolist())):
                        tok2d[i, :b - a] = tokens[a:b]
                    g['tokens2d'] = tok2d.numpy()
                    g[f'logits2d_{tag}'] = f32(model(tok2d))
                    g[f'logprob2d_packedin_{tag}'] = f32(model.predict_log_prob(
                        tokens, (cu, max_len), pad_output=True,
                        pad_indices=torch.cat([torch.arange(i * max_len, i * max_len + (b - a))
                                               for i, (a, b) in enumerate(zip(cu[:-1].tolist(), cu[1:].tolist()))])))
        # the bf16 arrays in a companion file (golden_util.load_golden merges the two): each file stays under 1 MiB
        bf16 = {k: v for k, v in g.items() if k.endswith('_bf16')}
        np.savez_compressed(os.path.join(HERE, fname), **{k: v for k, v in g.items() if k not in bf16})
        np.savez_compressed(os.path.join(HERE, fname[:-len('.npz')] + '_bf16.npz'), **bf16)
        return g

    run_model_fixture('g1_esm2_tiny.npz', 'esm2', 2, 64, 4, seed=11, lengths=[5, 26, 61],
                      mask_at=(3, 40), with_padded=True, layers_arg=[0])

    # ---- G2 README example on ESM2-8M dims (BASELINE config 1) -------------
    t2, idx2, cu2, ml2 = tokenize_unpad(readme, alphabet=Alphabet)
    g2 = {'tokens': t2.numpy(), 'cu_lens': cu2.numpy(), 'max_len': ml2, 'seed': 8,
          'tokens2d': tokenize(readme, alphabet=Alphabet).numpy()}
    for dt, tag in ((torch.float32, 'f32'), (torch.bfloat16, 'bf16')):
        with exact_cpu_gemms(dt == torch.bfloat16):
            model = build_ref_model(ref, syn, 'esm2', 6, 320, 20, 8, dt)
            g2[f'logprob_{tag}'] = f32(model.predict_log_prob(t2, (cu2, ml2)))
            g2[f'logprob2d_{tag}'] = f32(model.predict_log_prob(torch.from_numpy(g2['tokens2d'])))
    # from_pretrained round trip through the reference loader on our checkpoint file
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        path = syn.write_checkpoint(os.path.join(td, '8M.safetensors'), 'esm2_8m', seed=8)
        m = ref.ESM.from_pretrained(path)
        with exact_cpu_gemms():
            lp = m.predict_log_prob(t2, (cu2, ml2))
        assert np.array_equal(bits(lp), g2['logprob_bf16']), 'from_pretrained != direct build'
    np.savez_compressed(os.path.join(HERE, 'g2_esm2_8m_readme.npz'), **g2)

    # ---- G3 one ESM2-650M-width layer (E=1280,H=20,d=64), varlen rows ------
    sub = np.r_[0:3, 35:39, 105:108, 297:300]
    run_model_fixture('g3_esm2_650m_layer.npz', 'esm2', 1, 1280, 20, seed=3,
                      lengths=[37, 70, 193], tap_rows=sub)
    # ---- G3b one ESM2-150M-width layer (d=32) -------------------------------
    run_model_fixture('g3b_esm2_150m_layer.npz', 'esm2', 1, 640, 20, seed=4,
                      lengths=[130, 9, 61], tap_rows=np.r_[0:4, 127:133, 137:141, 196:200])

    # ---- G4 ESM-C: tiny full model + one 300M-width layer -------------------
    run_model_fixture('g4_esmc_tiny.npz', 'esmc', 2, 128, 2, seed=21, lengths=[7, 33, 50],
                      mask_at=(2,), with_padded=True)
    run_model_fixture('g4b_esmc_300m_layer.npz', 'esmc', 1, 960, 15, seed=22,
                      lengths=[45, 150, 5], tap_rows=np.r_[0:4, 43:47, 192:200])
    print('golden fixtures written to', HERE)
    for fn in sorted(os.listdir(HERE)):
        print(f'  {fn:32s} {os.path.getsize(os.path.join(HERE, fn)) / 1024:8.1f} KiB')


if __name__ == '__main__':
    main()
