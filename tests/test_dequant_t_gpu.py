"""The transposing expansion of quantised weights (include/esme_hip_dequant_t.h) on the device: dequantize_*_t(...) against
dequantize_*(...).t().contiguous() with torch.equal -- it is the same arithmetic, so there is no tolerance.  Shapes around the
128 x 64 tile (one element, one row short of a slot, of a tile, one past it, several tiles, tails in both directions), both codebooks,
random weights and one matrix that holds every code value and an all-zero block, `out` as a column view of a canary-filled wider buffer,
`codes` as a row slice of a larger packed tensor (as q / k / v are), and two runs bit-equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPES = [(1, 64), (63, 64), (64, 64), (65, 128), (192, 320), (320, 192), (129, 1280)]
SHAPES8 = SHAPES + [(7, 8), (65, 72)]
CANARY = 0x5A5A


def _weight(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).to(DEV)


def _check_t(plain, transposed, N, K):
    """transposed(out) against plain().t(): a fresh result, a canary-framed column view, and a second run."""
    want = plain().t().contiguous()
    got = transposed(None)
    assert got.shape == (K, N) and got.dtype == torch.bfloat16
    assert torch.equal(got, want), f'{int((got != want).sum())} of {want.numel()} elements differ'
    ld = (N + 7) // 8 * 8 + 24
    frame = torch.full((K + 5, ld), CANARY, dtype=torch.int16, device=DEV)
    view = frame.view(torch.bfloat16)[:K, 8:8 + N]                  # ldo > N, 16-byte aligned, not the allocation's base
    assert transposed(view) is view
    assert torch.equal(view, want)
    check = frame.clone()
    check[:K, 8:8 + N] = CANARY
    assert bool((check == CANARY).all()), 'canary columns / rows past K were written'
    again = transposed(None)
    assert torch.equal(again, got)


@pytest.mark.parametrize('quant_type', ('fp4', 'nf4'))
@pytest.mark.parametrize('N,K', SHAPES)
def test_4bit_transposed_equals_plain(N, K, quant_type):
    from esme import _hip, _hip_dequant_t as HT
    from esme.quantization import codebook_of
    cb = codebook_of(quant_type)
    codes, absmax = _hip.quantize_4bit(_weight(N, K, N + K), cb)
    _check_t(lambda: _hip.dequantize_4bit(codes, absmax, cb), lambda out: HT.dequantize_4bit_t(codes, absmax, cb, out=out), N, K)


@pytest.mark.parametrize('N,K', SHAPES8)
def test_8bit_transposed_equals_plain(N, K):
    from esme import _hip, _hip_dequant_t as HT
    codes, scale = _hip.quantize_8bit(_weight(N, K, N + K + 1))
    _check_t(lambda: _hip.dequantize_8bit(codes, scale), lambda out: HT.dequantize_8bit_t(codes, scale, out=out), N, K)


@pytest.mark.parametrize('quant_type', ('fp4', 'nf4'))
def test_4bit_every_code_and_a_zero_block(quant_type):
    from esme import _hip, _hip_dequant_t as HT
    from esme.quantization import codebook_of
    cb = codebook_of(quant_type)
    N, K = 130, 128
    codes = (torch.arange(N * K // 2, dtype=torch.int64) * 7 % 256).to(torch.uint8).view(N, K // 2).to(DEV)      # every byte value, i.e. every code in both nibbles
    assert codes.unique().numel() == 256
    absmax = (0.01 + torch.rand(N, K // 64, generator=torch.Generator().manual_seed(3))).to(DEV)
    absmax[5, 1] = 0.0                                                                                          # an all-zero block
    absmax[129, 0] = 0.0
    want = _hip.dequantize_4bit(codes, absmax, cb)
    assert want.float().unique().numel() >= 16 and not bool(want[5, 64:].any()) and bool(want[5, :64].any())
    got = HT.dequantize_4bit_t(codes, absmax, cb)
    assert torch.equal(got, want.t()) and not bool(got[64:, 5].any())


def test_8bit_every_code_and_a_zero_row():
    from esme import _hip, _hip_dequant_t as HT
    N, K = 130, 256
    codes = (torch.arange(N * K, dtype=torch.int64) * 3 % 256 - 128).to(torch.int8).view(N, K).to(DEV)
    assert codes.unique().numel() == 256
    scale = (0.01 + torch.rand(N, generator=torch.Generator().manual_seed(4))).to(DEV)
    scale[7] = 0.0
    want = _hip.dequantize_8bit(codes, scale)
    got = HT.dequantize_8bit_t(codes, scale)
    assert torch.equal(got, want.t()) and not bool(got[:, 7].any()) and bool(got[:, 8].any())


@pytest.mark.parametrize('bits', (4, 8))
def test_codes_as_a_row_slice_of_a_packed_tensor(bits):
    """q / k / v hold row slices of one packed code tensor: `codes` then does not start at its allocation's base."""
    from esme import _hip, _hip_dequant_t as HT
    from esme.quantization import FP4_CODEBOOK
    E = 192
    w = _weight(3 * E, E, 11)
    if bits == 4:
        codes, absmax = _hip.quantize_4bit(w, FP4_CODEBOOK)
    else:
        codes, absmax = _hip.quantize_8bit(w)
    for i in range(3):
        c, a = codes[i * E:(i + 1) * E], absmax[i * E:(i + 1) * E]
        assert c.is_contiguous() and (i == 0 or c.data_ptr() != codes.data_ptr())
        if bits == 4:
            want, got = _hip.dequantize_4bit(c, a, FP4_CODEBOOK), HT.dequantize_4bit_t(c, a, FP4_CODEBOOK)
        else:
            want, got = _hip.dequantize_8bit(c, a), HT.dequantize_8bit_t(c, a)
        assert torch.equal(got, want.t()), i


def test_the_modules_expand_their_own_codes():
    from esme.nn import Linear
    from esme.quantization import Linear4bit, Linear8bit
    lin = Linear(128, 192, bias=True).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(_weight(192, 128, 5))
    for q in (Linear4bit.from_linear(lin, 'fp4'), Linear4bit.from_linear(lin, 'nf4'), Linear8bit.from_linear(lin)):
        wt = q.dequantize_t()
        assert wt.shape == (128, 192) and torch.equal(wt, q.dequantize().t())
        scratch = torch.zeros(128 * 192 + 64, dtype=torch.bfloat16, device=DEV)
        assert torch.equal(q.dequantize_t(out=scratch[:128 * 192].view(128, 192)), wt) and not bool(scratch[128 * 192:].any())
