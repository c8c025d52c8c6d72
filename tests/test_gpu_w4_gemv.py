"""The NF4 decode-weight kernels: ops.quantize_blocks_nf4 (mp_quantize_blocks_nf4_bf16: 4-bit codes into QLoRA's table, one fp32 absmax per
64 weights, bit-equal to the torch restatement tests/nf4_ref.py) and ops.gemv_w4 (mp_gemv_w4_bf16: bf16 activations against those codes, the
table rounded to bf16, mp_gemv_bf16's epilogues).

Most of this file needs no tolerance.  On "grid" weights W = bf16(NF4[c]) * 2^e_b (one +-1 per block of 64, e_b in {-7, -6}: exact in bf16)
the quantiser must return c and 2^e_b.  bf16 table entries are multiples of 2^-11, so with integer x in [-4, 4] every partial sum is a
multiple of 2^-18 below 1024 * 4 * 2^-6 = 64 at K <= 1024: at most 24 significant bits, every association of the fp32 sum is exact, and the
kernel must EQUAL the float64 reference rounded once, and ops.gemv on the bf16 grid weights, in every form whose epilogue is plain roundings
(bf16, fp32, residual, the indexed combine).  For longer K the codes are ternary {0, 7, 15} = {-1, 0, 1}: sums are integers times 2^-7 and
stay exact up to K = 11008.  Random operands then check the kernel's own rounding against fp32 x @ dequant^T — the quantisation error is in
the reference — at the tolerances of tests/test_gpu_w8_gemv.py, the project's own for this kernel family."""
import math

import pytest
import torch

import nf4_ref as R
from oracle import ops as O

pytestmark = pytest.mark.gpu

BF16_EPS = 2.0 ** -8


def _bf(x):
    return x.to(torch.bfloat16)


def _report(name, got, ref, rtol, atol):
    got, ref = got.float().cpu(), ref.float().cpu()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    msg = f"{name}: max|err|={err.max().item():.4e}, ref absmax={ref.abs().max().item():.4e}, bad={int(bad.sum())}/{bad.numel()}"
    print(msg)
    assert not bad.any(), msg


def _grid(g, *shape, ternary=False):
    """Grid weights [..., N, K] -> (w bf16, code uint8 [..., N, K], absmax fp32 [..., N, K/64]): every block holds one +-1 (code 15 or 0)."""
    nb = shape[-1] // 64
    bshape = shape[:-1] + (nb, 64)
    if ternary:
        c = torch.tensor([0, 7, 15], dtype=torch.uint8)[torch.randint(0, 3, bshape, generator=g)]
    else:
        c = torch.randint(0, 16, bshape, generator=g, dtype=torch.uint8)
    at = torch.randint(0, 64, bshape[:-1] + (1,), generator=g)
    c.scatter_(-1, at, (torch.randint(0, 2, bshape[:-1] + (1,), generator=g) * 15).to(torch.uint8))
    absmax = torch.pow(torch.tensor(2.0), torch.randint(-7, -5, bshape[:-1], generator=g).float())
    exact = (R.NF4_BF16[c.long()] * absmax.unsqueeze(-1)).flatten(-2)            # 8 bits times a power of two: exact in fp32 and in bf16
    w = exact.to(torch.bfloat16)
    assert torch.equal(w.float(), exact)
    return w, c.flatten(-2), absmax


def _ints(g, M, K):
    return _bf(torch.randint(-4, 5, (M, K), generator=g).float())


def _quantise_grid(dev, w, c, absmax):
    """The quantiser on grid weights returns the grid: -> (codes, absmax) on the device."""
    from medplib_amd import ops
    codes, am = ops.quantize_blocks_nf4(w.to(dev))
    assert torch.equal(codes.cpu(), R.pack(c)) and torch.equal(am.cpu(), absmax), tuple(w.shape)
    return codes, am


# ------------------------------------------------------------------------------------------------ the quantiser
def test_quantiser_is_bit_equal_to_the_reference(dev):
    from medplib_amd import ops
    g = torch.Generator().manual_seed(171)
    cases = [_bf(torch.randn(N, K, generator=g) * 0.05) for N, K in ((7, 64), (100, 320), (5, 11008))]
    z = _bf(torch.randn(6, 128, generator=g)); z[2, 64:] = 0                          # an all-zero block
    neg = _bf(torch.randn(4, 192, generator=g) * 0.1); neg[1, 64 + 17] = -3.0         # a block whose absmax is a negative entry
    cases += [z, neg, _bf(torch.randn(3, 64, 256, generator=g) * 0.02)]               # and an expert tensor
    for w in cases:
        codes, absmax = ops.quantize_blocks_nf4(w.to(dev))
        rc, ra = R.quant_ref(w)
        K = w.shape[-1]
        assert codes.dtype == torch.uint8 and codes.shape == w.shape[:-1] + (K // 2,)
        assert absmax.dtype == torch.float32 and absmax.shape == w.shape[:-1] + (K // 64,)
        assert torch.equal(absmax.cpu(), ra), tuple(w.shape)
        assert torch.equal(codes.cpu(), rc), tuple(w.shape)
    codes, absmax = ops.quantize_blocks_nf4(z.to(dev))
    assert (codes[2, 32:].cpu() == 0x77).all() and float(absmax[2, 1]) == 0.0, "a zero block: codes 7, absmax 0"
    codes, absmax = ops.quantize_blocks_nf4(neg.to(dev))
    assert float(absmax[1, 1]) == 3.0 and int(R.unpack(codes.cpu())[1, 64 + 17]) == 0, "the negative absmax entry is code 0"
    for shape in ((64, 512), (2, 32, 1024)):
        _quantise_grid(dev, *_grid(g, *shape))


def test_quantiser_decides_strictly_at_every_threshold(dev):
    """No bf16 weight lands exactly on a threshold (tests/test_w4_abi.py shows that exhaustively), so the nearest bf16 values on either
    side of each: below -> code i, above -> code i + 1; with block absmax 1 the scaled value is the weight itself."""
    from medplib_amd import ops
    t = R.THRESHOLDS
    b = t.to(torch.bfloat16)
    assert not torch.equal(b.float(), t)
    up = (b.view(torch.int16) + torch.where(b.float() > 0, 1, -1).to(torch.int16)).view(torch.bfloat16)
    dn = (b.view(torch.int16) - torch.where(b.float() > 0, 1, -1).to(torch.int16)).view(torch.bfloat16)
    lo = torch.where(b.float() < t, b, dn)
    hi = torch.where(b.float() > t, b, up)
    assert (lo.float() < t).all() and (hi.float() > t).all() and (hi.float() - lo.float() < 2.0 ** -7).all()
    w = torch.zeros(2, 64, dtype=torch.bfloat16)
    w[:, 0] = 1.0
    w[0, 1:16], w[1, 1:16] = lo, hi
    codes, absmax = ops.quantize_blocks_nf4(w.to(dev))
    code = R.unpack(codes.cpu()).long()
    assert torch.equal(code[0, 1:16], torch.arange(15)) and torch.equal(code[1, 1:16], torch.arange(1, 16)) and (absmax.cpu() == 1).all()
    assert torch.equal(codes.cpu(), R.quant_ref(w)[0])


def test_quantiser_writes_nothing_outside_its_rows(dev):
    """Padded ldw / ldc / lda with sentinel-filled guard bands: only [rows, K/2] and [rows, K/64] are written."""
    from medplib_amd import ops
    from medplib_amd._lib import lib
    g = torch.Generator().manual_seed(173)
    rows, K, ldw, ldc, lda = 9, 320, 336, 176, 7
    w = _bf(torch.randn(rows, ldw, generator=g))
    wd = w.to(dev)
    codes = torch.full((rows + 2, ldc), 0xAB, dtype=torch.uint8, device=dev)
    absmax = torch.full((rows + 2, lda), -123.0, dtype=torch.float32, device=dev)
    lib().call("mp_quantize_blocks_nf4_bf16", wd.data_ptr(), ldw, rows, K, codes[1].data_ptr(), ldc, absmax[1].data_ptr(), lda,
               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rc, ra = R.quant_ref(w[:, :K])
    codes, absmax = codes.cpu(), absmax.cpu()
    assert torch.equal(codes[1:rows + 1, :K // 2], rc) and torch.equal(absmax[1:rows + 1, :K // 64], ra)
    codes[1:rows + 1, :K // 2] = 0xAB
    absmax[1:rows + 1, :K // 64] = -123.0
    assert (codes == 0xAB).all() and (absmax == -123.0).all()


# ------------------------------------------------------------------------------------------------ exact GEMV on the grid
def _exact_shared(dev, g, M, N, K, ternary=False):
    from medplib_amd import ops
    w, c, am = _grid(g, N, K, ternary=ternary)
    x, res = _ints(g, M, K), _bf(torch.randn(M, N, generator=g))
    y32 = (x.double() @ w.double().T).float()                  # exact: at most 24 significant bits (module docstring)
    assert torch.equal(y32.double(), x.double() @ w.double().T)
    xd, wd, rd = x.to(dev), w.to(dev), res.to(dev)
    codes, absmax = _quantise_grid(dev, w, c, am)
    tag = (M, N, K)
    got = ops.gemv_w4(xd, codes, absmax)
    assert torch.equal(got.cpu(), y32.to(torch.bfloat16)), tag
    assert torch.equal(got, ops.gemv(xd, wd)), tag
    got32 = ops.gemv_w4(xd, codes, absmax, out_dtype=torch.float32)
    assert torch.equal(got32.cpu(), y32) and torch.equal(got32, ops.gemv(xd, wd, out_dtype=torch.float32)), tag
    gotr = ops.gemv_w4(xd, codes, absmax, residual=rd)
    assert torch.equal(gotr.cpu(), (y32.to(torch.bfloat16).float() + res.float()).to(torch.bfloat16)), tag
    assert torch.equal(gotr, ops.gemv(xd, wd, residual=rd)), tag
    assert torch.equal(ops.gemv_w4(xd, codes, absmax, residual=rd), gotr), "a second launch gives the same bits"


@pytest.mark.parametrize("M,N,K", [(1, 5, 64), (3, 1000, 1024), (2, 256, 320), (6, 192, 640)])
def test_shared_form_is_exact_on_grid_operands(dev, M, N, K):
    """K = 64: one block, two lanes, a ragged N; N = 1000 is ragged over a workgroup's sixteen rows; K = 320 / 640 are a single ragged step of
    either load width; M = 6 is two passes."""
    _exact_shared(dev, torch.Generator().manual_seed(173 + M), M, N, K)


@pytest.mark.parametrize("M,N,K", [(1, 4096, 4096), (1, 4096, 11008), (1, 1000, 4160), (3, 768, 2112)])
def test_long_k_is_exact_on_ternary_grid_operands(dev, M, N, K):
    """N <= 4096, K >= 4096, one row: the K-split form (K = 4096: one step in each of the four parts; K = 11008: 10.75 steps; K = 4160: one
    block past four steps).  (3, 768, 2112): the shared form with 8-byte loads, two steps and one block."""
    _exact_shared(dev, torch.Generator().manual_seed(179), M, N, K, ternary=True)


@pytest.mark.parametrize("E,N,K,M,idx,keep,ternary", [(3, 256, 512, 4, (2, 0, 1, 2), (0, 3, -1, 1), False),
                                                      (2, 4096, 11008, 3, (1, 0, 1), (0, -1, 1), True)])
def test_indexed_form_is_exact_on_grid_operands(dev, E, N, K, M, idx, keep, ternary):
    """The expert form (the wave-per-four-rows kernel at K = 512, the K-split one at 4096 x 11008): row m streams expert idx[m]'s codes and
    absmax; combine weight on the bf16-rounded output, then the residual; a dropped row keeps its residual bits exactly."""
    from medplib_amd import ops
    g = torch.Generator().manual_seed(183)
    w, c, am = _grid(g, E, N, K, ternary=ternary)
    x, res = _ints(g, M, K), _bf(torch.randn(M, N, generator=g))
    rs = torch.tensor([0.7, 0.9, 0.55, 0.6][:M])
    idx_t, keep_t = torch.tensor(idx, dtype=torch.int32), torch.tensor(keep, dtype=torch.int32)
    rows = []
    for m in range(M):
        y32 = (x[m].double() @ w[idx[m]].double().T).float()
        rows.append(res[m] if keep[m] < 0 else (rs[m] * y32.to(torch.bfloat16).float() + res[m].float()).to(torch.bfloat16))
    ref = torch.stack(rows)
    wd = w.to(dev)
    codes, absmax = _quantise_grid(dev, w, c, am)
    kw = dict(residual=res.to(dev), w_index=idx_t.to(dev), row_scale=rs.to(dev), row_keep=keep_t.to(dev))
    got = ops.gemv_w4(x.to(dev), codes, absmax, **kw)
    assert torch.equal(got.cpu(), ref)
    dropped = keep.index(-1)
    assert torch.equal(got[dropped].cpu(), res[dropped]), "a capacity-dropped row keeps the residual stream exactly"
    assert torch.equal(got, ops.gemv(x.to(dev), wd, **kw))
    assert torch.equal(ops.gemv_w4(x.to(dev), codes, absmax, **kw), got), "a second launch gives the same bits"


@pytest.mark.parametrize("M", [1, 8])
def test_table_sweep_every_code_at_every_nibble_position(dev, M):
    """One-hot x, fp32 output: y[n] == fp32(bf16(NF4[c]) * absmax) exactly, for every code at every position of a lane's load.  K = 64 is two
    lanes of a 16-byte load (one x row) and four of an 8-byte load (M = 8: two passes of four rows); row n holds code (n + p) % 16 at p."""
    from medplib_amd import ops
    g = torch.Generator().manual_seed(191)
    N, K = 16, 64
    code = ((torch.arange(N).unsqueeze(1) + torch.arange(K).unsqueeze(0)) % 16).to(torch.uint8)
    absmax = (torch.rand(N, 1, generator=g) + 0.25).float()
    codes, am = R.pack(code).to(dev), absmax.to(dev)
    for p0 in range(0, K, M):
        x = torch.zeros(M, K)
        x[torch.arange(M), p0 + torch.arange(M)] = 1.0
        got = ops.gemv_w4(_bf(x).to(dev), codes, am, out_dtype=torch.float32).cpu()
        want = torch.stack([R.NF4_BF16[code[:, p0 + m].long()] * absmax[:, 0] for m in range(M)])
        assert torch.equal(got, want), p0


# ------------------------------------------------------------------------------------------------ random operands
def test_random_operands_within_the_bf16_kernels_tolerances(dev):
    """Random x and W: the reference is fp32 x @ dequant^T (bf16-rounded table times the block absmax) through the reference epilogue, so the
    quantisation error is on both sides and the kernel owes its own rounding only — at test_gpu_w8_gemv.py's shapes and tolerances (its
    K = 4112 is no multiple of 64: 4160 here, one block past four steps of the K-split form)."""
    from medplib_amd import ops
    g = torch.Generator().manual_seed(189)
    for M, N, K in ((1, 768, 512), (3, 1000, 1024), (2, 256, 320), (6, 192, 640), (1, 4096, 4096), (1, 1000, 4160)):
        x = _bf(torch.randn(M, K, generator=g)); w = _bf(torch.randn(N, K, generator=g) * 0.05); res = _bf(torch.randn(M, N, generator=g))
        codes, absmax = ops.quantize_blocks_nf4(w.to(dev))
        ref = O.linear(x.float(), R.dequant_ref(codes, absmax))
        _report(f"gemv_w4 {M}x{N}x{K}", ops.gemv_w4(x.to(dev), codes, absmax), ref, rtol=2 * BF16_EPS, atol=1e-3 * math.sqrt(K))
        _report(f"gemv_w4 f32 out {M}x{N}x{K}", ops.gemv_w4(x.to(dev), codes, absmax, out_dtype=torch.float32), ref, rtol=1e-4, atol=2e-3)
        _report(f"gemv_w4 residual {M}x{N}x{K}", ops.gemv_w4(x.to(dev), codes, absmax, residual=res.to(dev)),
                ref.to(torch.bfloat16).float() + res.float(), rtol=2 * BF16_EPS, atol=2e-2)
    # SwiGLU pairing over the interleaved gate|up rows (a block lies inside one row, so the format is indifferent to the interleave)
    M, ff, K = 2, 320, 1024
    x = _bf(torch.randn(M, K, generator=g)).to(dev)
    wg = _bf(torch.randn(ff, K, generator=g) * 0.1).to(dev); wu = _bf(torch.randn(ff, K, generator=g) * 0.1).to(dev)
    qg, qu = ops.quantize_blocks_nf4(wg), ops.quantize_blocks_nf4(wu)
    codes, absmax = ops.quantize_blocks_nf4(ops.swiglu_interleave(wg, wu))
    ref = O.swiglu(O.linear(x.float().cpu(), R.dequant_ref(*qg)), O.linear(x.float().cpu(), R.dequant_ref(*qu)))
    _report("gemv_w4 swiglu pair", ops.gemv_w4(x, codes, absmax, act=ops.ACT_SWIGLU_PAIR), ref, rtol=3 * BF16_EPS, atol=2e-2)
    # the indexed SwiGLU at E = 2, then the row_scale form on its output's shape
    E, M = 2, 3
    wg = _bf(torch.randn(E, ff, K, generator=g) * 0.1).to(dev); wu = _bf(torch.randn(E, ff, K, generator=g) * 0.1).to(dev)
    wi = torch.stack([ops.swiglu_interleave(wg[e], wu[e]) for e in range(E)])
    codes, absmax = ops.quantize_blocks_nf4(wi)
    x = _bf(torch.randn(M, K, generator=g)).to(dev)
    idx = torch.tensor([1, 0, 1], dtype=torch.int32)
    dg, du = R.dequant_ref(*ops.quantize_blocks_nf4(wg)), R.dequant_ref(*ops.quantize_blocks_nf4(wu))
    ref = torch.stack([O.swiglu(O.linear(x[m:m + 1].float().cpu(), dg[idx[m]]), O.linear(x[m:m + 1].float().cpu(), du[idx[m]]))[0] for m in range(M)])
    got = ops.gemv_w4(x, codes, absmax, act=ops.ACT_SWIGLU_PAIR, w_index=idx.to(dev))
    _report("gemv_w4 indexed swiglu", got, ref, rtol=3 * BF16_EPS, atol=2e-2)
    assert torch.equal(ops.gemv_w4(x, codes, absmax, act=ops.ACT_SWIGLU_PAIR, w_index=idx.to(dev)), got), "a second launch gives the same bits"
    N, K = 256, 512
    x = _bf(torch.randn(M, K, generator=g)); w = _bf(torch.randn(E, N, K, generator=g) * 0.05); res = _bf(torch.randn(M, N, generator=g))
    rs, keep = torch.tensor([0.7, 0.9, 0.55]), torch.tensor([0, 2, 1], dtype=torch.int32)
    codes, absmax = ops.quantize_blocks_nf4(w.to(dev))
    dq = R.dequant_ref(codes, absmax)
    ref = torch.stack([res[m].float() + rs[m] * (x[m].float() @ dq[idx[m]].t()).to(torch.bfloat16).float() for m in range(M)])
    got = ops.gemv_w4(x.to(dev), codes, absmax, residual=res.to(dev), w_index=idx.to(dev), row_scale=rs.to(dev), row_keep=keep.to(dev))
    _report("gemv_w4 experts row_scale", got, ref, rtol=3 * BF16_EPS, atol=2e-2)
