"""float64 reference, per-element error bounds and a CPU emulation for the weight-gradient GEMM (csrc/gemm_wgrad.hip).

`reference_wgrad` is dW = dy^T x and db = the column sums of dy in float64 on the operands the kernel is handed.  `wgrad_bound` is
the sum of the kernel's rounding steps, built from tests/error_bounds.py's constants: the fp32 accumulation of exact bf16 products
over the rows of each chunk (`dot_term`, the statistical MFMA form), the ordered fp32 sum of the chunks' partials, and the one
rounding to the output dtype; the same for db, whose terms are exact bf16 values added in fp32.  `split` restates the header's row
partition (a function of the shape alone).  `emulate_wgrad` is a float32 CPU emulation of the kernel's order of operations with
switches for defects; tests/test_gemm_wgrad_cpu.py checks that the bound accepts the correct emulation and rejects each defect, on
the shapes tests/test_gemm_wgrad_gpu.py runs.  Nothing here is tuned to a GPU run.
"""
import torch

import error_bounds as eb

TILE, STAGE, TARGET, MIN_ROWS, MAX_CHUNKS, MAX_WORK = 128, 64, 512, 256, 64, 2048      # kWgTile, kWgRows, kWgTarget, kWgMinRows, kWgMaxChunks, kWgMaxWork (gemm_wgrad.hip)

MS = (0, 1, 63, 64, 65, 200, 4099)
NKS = ((64, 64), (192, 64), (64, 320), (320, 192))
DEFECTS = ('untransposed', 'drop_tail', 'row_past_m', 'skip_last_partial', 'bf16_partials', 'db_from_x')
FMT = {'bf16': torch.bfloat16, 'fp32': torch.float32}


def _cdiv(a, b):
    return -(-a // b)


def split(M, N, K):
    """(rows of a chunk, chunks): include/esme_hip_gemm_wgrad.h."""
    tiles = _cdiv(N, TILE) * _cdiv(K, TILE)
    most = min(MAX_CHUNKS, max(1, MAX_WORK // tiles), _cdiv(M, MIN_ROWS))
    c, best = 1, (0, 1)
    for i in range(1, most + 1):                                         # the smallest c with the fullest last round of TARGET workgroups
        a = tiles * i
        b = TARGET * _cdiv(a, TARGET)
        if a * best[1] > best[0] * b:
            c, best = i, (a, b)
    rows = max(STAGE, _cdiv(_cdiv(M, c), STAGE) * STAGE)
    return rows, max(1, _cdiv(M, rows))


def workspace_bytes(M, N, K):
    chunks = split(M, N, K)[1]
    return 0 if chunks == 1 else chunks * (N * K + N) * 4


def defect_applies(defect, M, N, K):
    """Whether `defect` changes anything at this shape: a tail exists only when M is no multiple of the 64-row stage, partials only
    with more than one chunk, and with no row at all only the row past M contributes."""
    if defect == 'row_past_m':
        return True
    if M == 0:
        return False
    if defect == 'drop_tail':
        return M % STAGE != 0
    if defect in ('skip_last_partial', 'bf16_partials'):
        return split(M, N, K)[1] > 1
    return True


def make_operands(M, N, K, seed, device='cpu', pad=24):
    """dy (M, N) and x (M, K) bfloat16 as column views (first column 8) of buffers with row strides N + pad and K + pad and one
    more row than M, which `emulate_wgrad(defect='row_past_m')` reads and the kernel must not."""
    g = torch.Generator().manual_seed(seed)
    by = torch.randn(M + 1, N + pad, generator=g).to(torch.bfloat16).to(device)
    bx = torch.randn(M + 1, K + pad, generator=g).to(torch.bfloat16).to(device)
    return by[:M, 8:8 + N], bx[:M, 8:8 + K], by, bx


def reference_wgrad(dy, x):
    """(dW (N, K), db (N)) float64."""
    dy64 = dy.double()
    return dy64.T @ x.double(), dy64.sum(0)


def wgrad_bound(dy, x, out_fmt):
    """(bound of dW (N, K), bound of db (N)) float64 for |kernel - reference_wgrad|, `out_fmt` 'bf16' or 'fp32'."""
    M, N = dy.shape
    K = x.shape[1]
    rows, chunks = split(M, N, K)
    dy64, x64 = dy.double(), x.double()
    dev = dy.device
    preW = torch.zeros(N, K, dtype=torch.float64, device=dev)
    preb = torch.zeros(N, dtype=torch.float64, device=dev)
    magW, magb = torch.zeros_like(preW), torch.zeros_like(preb)
    for c in range(chunks):
        yc, xc = dy64[c * rows:(c + 1) * rows], x64[c * rows:(c + 1) * rows]
        if yc.shape[0] == 0:
            continue
        preW += eb.dot_term(yc.T, xc.T)                                  # the chunk's MFMA chain over its rows: exact products, fp32 accumulation
        preb += eb.dot_term(yc.T, torch.ones(1, yc.shape[0], dtype=torch.float64, device=dev)).squeeze(1)      # the same against ones
        magW += (yc.T @ xc).abs()
        magb += yc.sum(0).abs()
    preW += (chunks - 1) * eb.U32 * magW                                 # wgrad_reduce_kernel: chunks - 1 fp32 adds in chunk order
    preb += (chunks - 1) * eb.U32 * magb
    rW, rb = reference_wgrad(dy, x)
    return preW + eb.out_round(rW, preW, out_fmt), preb + eb.out_round(rb, preb, out_fmt)      # one rounding to the output dtype


def worst(got, ref, bound):
    """max of err / bound over the tensors given (0 / 0 counts as 0)"""
    w = 0.0
    for g, r, b in zip(got, ref, bound):
        if g is None or g.numel() == 0:
            continue
        assert bool(torch.isfinite(g.double()).all()), 'non-finite output'
        err = (g.double() - r.double().to(g.device)).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / b.double().to(g.device))
        w = max(w, float(ratio.max()))
    return w


def emulate_wgrad(dy, x, out_fmt, defect=None, past=None):
    """float32 emulation of esme_hip_gemm_wgrad on the CPU: (dW, db) in the output dtype.  `defect`: None or one of DEFECTS --
    'untransposed' (the K x N product laid out as N x K), 'drop_tail' (the rows of the last chunk past its last full 64-row stage
    dropped), 'row_past_m' (row M counted: `past` = (that row of dy's buffer, of x's buffer)), 'skip_last_partial' (the last chunk's
    partial left out of the sum), 'bf16_partials' (partials rounded to bfloat16 before the reduce), 'db_from_x' (db = column sums
    of x)."""
    assert defect is None or defect in DEFECTS, defect
    M, N = dy.shape
    K = x.shape[1]
    rows, chunks = split(M, N, K)
    y32, x32 = dy.float().cpu(), x.float().cpu()
    if defect == 'row_past_m':
        y32, x32 = torch.cat((y32, past[0].float().cpu().view(1, N))), torch.cat((x32, past[1].float().cpu().view(1, K)))
    partsW, partsb = [], []
    for c in range(chunks):
        a, b = c * rows, min(M, (c + 1) * rows)
        if c == chunks - 1:
            if defect == 'drop_tail':
                b = a + (b - a) // STAGE * STAGE
            if defect == 'row_past_m':
                b += 1
        yc, xc = y32[a:b], x32[a:b]
        pw = (xc.T @ yc).reshape(N, K) if defect == 'untransposed' else yc.T @ xc
        pb = (xc[:, torch.arange(N) % K] if defect == 'db_from_x' else yc).sum(0)
        if defect == 'bf16_partials':
            pw, pb = pw.to(torch.bfloat16).float(), pb.to(torch.bfloat16).float()
        partsW.append(pw)
        partsb.append(pb)
    if defect == 'skip_last_partial':
        partsW, partsb = partsW[:-1], partsb[:-1]
    dW, db = partsW[0], partsb[0]
    for pw, pb in zip(partsW[1:], partsb[1:]):                           # chunk order
        dW, db = dW + pw, db + pb
    return dW.to(FMT[out_fmt]), db.to(FMT[out_fmt])
