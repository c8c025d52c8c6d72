"""The 8-bit decode-weight kernels: ops.quantize_rows_w8 (mp_quantize_rows_w8_bf16, row-wise absmax int8 codes + fp32 scales, bit-equal to
its fp32 formula restated in torch) and ops.gemv_w8 (mp_gemv_w8_bf16, bf16 activations against those codes with mp_gemv_bf16's epilogues).

Most of this file needs no tolerance.  On "grid" weights W = c * 2^e (c an integer in [-127, 127] with one +-127 per row, e per row in
[-12, -5]: exact in bf16) the quantiser must return c and 2^e, and with integer x in [-4, 4] every partial sum is an integer below
127 * 4 * K = 5.6 M < 2^24 at K = 11008, so every association of the fp32 sum is exact: the kernel must EQUAL the float64 reference rounded
once, and ops.gemv on the bf16 grid weights, in every form whose epilogue is plain roundings (bf16, fp32, residual, the indexed combine).
Random operands then check the kernel's own rounding against fp32 x @ (code * scale)^T — the quantisation error is in the reference — at the
tolerances of test_gemv_decode_projections / test_gemv_ksplit_narrow_projections."""
import math

import pytest
import torch

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


def _quant_ref(w):
    """The format, one fp32 operation per step in the order written: -> (codes int8, scale fp32) of w [..., K] bf16 on the CPU."""
    f = w.float()
    absmax = f.abs().amax(-1, keepdim=True)
    scale = absmax / torch.tensor(127.0)
    inv = torch.where(absmax > 0, torch.tensor(127.0) / absmax, torch.zeros_like(absmax))
    return torch.round(f * inv).to(torch.int8), scale.squeeze(-1)


def _grid(g, *shape):
    """Grid weights [..., N, K] -> (w bf16, c int16, e int64 [..., N])."""
    c = torch.randint(-127, 128, shape, generator=g, dtype=torch.int16)
    at = torch.randint(0, shape[-1], shape[:-1] + (1,), generator=g)
    sign = (torch.randint(0, 2, shape[:-1] + (1,), generator=g) * 2 - 1).to(torch.int16)
    c.scatter_(-1, at, 127 * sign)
    e = torch.randint(-12, -4, shape[:-1], generator=g)
    exact = c.float() * torch.pow(torch.tensor(2.0), e.float()).unsqueeze(-1)            # 7 bits times a power of two: exact in fp32 and in bf16
    w = exact.to(torch.bfloat16)
    assert torch.equal(w.float(), exact)
    return w, c, e


def _ints(g, M, K):
    return _bf(torch.randint(-4, 5, (M, K), generator=g).float())


def test_quantiser_is_bit_equal_to_its_fp32_formula(dev):
    from medplib_amd import ops
    g = torch.Generator().manual_seed(71)
    cases = [_bf(torch.randn(N, K, generator=g) * 0.05) for N, K in ((7, 16), (100, 320), (5, 11008))]
    z = _bf(torch.randn(6, 64, generator=g)); z[2] = 0                                # an all-zero row
    neg = _bf(torch.randn(4, 48, generator=g) * 0.1); neg[1, 17] = -3.0               # a row whose absmax is a negative entry
    cases += [z, neg, _bf(torch.randn(3, 64, 256, generator=g) * 0.02)]               # and an expert tensor
    for w in cases:
        codes, scale = ops.quantize_rows_w8(w.to(dev))
        rc, rs = _quant_ref(w)
        assert codes.dtype == torch.int8 and codes.shape == w.shape and scale.dtype == torch.float32 and scale.shape == w.shape[:-1]
        assert torch.equal(scale.cpu(), rs), tuple(w.shape)
        assert torch.equal(codes.cpu(), rc), tuple(w.shape)
        assert int(codes.cpu().abs().max()) <= 127
        # what the format promises: |W - code * scale| <= scale / 2, up to the fp32 rounding of the two products
        err = (w.double() - rc.double() * rs.double().unsqueeze(-1)).abs()
        assert (err <= rs.double().unsqueeze(-1) * (0.5 + 2.0 ** -16)).all()
    assert torch.equal(ops.quantize_rows_w8(z.to(dev))[0][2].cpu(), torch.zeros(64, dtype=torch.int8)) and float(_quant_ref(z)[1][2]) == 0.0
    assert int(ops.quantize_rows_w8(neg.to(dev))[0][1, 17]) == -127
    for shape in ((64, 512), (2, 32, 1024)):
        w, c, e = _grid(g, *shape)
        codes, scale = ops.quantize_rows_w8(w.to(dev))
        assert torch.equal(codes.cpu().to(torch.int16), c) and torch.equal(scale.cpu().double(), torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double()))


def _exact_shared(dev, g, M, N, K):
    from medplib_amd import ops
    w, c, e = _grid(g, N, K)
    x, res = _ints(g, M, K), _bf(torch.randn(M, N, generator=g))
    y32 = (x.double() @ w.double().T).float()                  # exact: every partial sum is an integer multiple of 2^e below 2^24 of them
    assert torch.equal(y32.double(), x.double() @ w.double().T)
    xd, wd, rd = x.to(dev), w.to(dev), res.to(dev)
    codes, scale = ops.quantize_rows_w8(wd)
    tag = (M, N, K)
    got = ops.gemv_w8(xd, codes, scale)
    assert torch.equal(got.cpu(), y32.to(torch.bfloat16)), tag
    assert torch.equal(got, ops.gemv(xd, wd)), tag
    got32 = ops.gemv_w8(xd, codes, scale, out_dtype=torch.float32)
    assert torch.equal(got32.cpu(), y32) and torch.equal(got32, ops.gemv(xd, wd, out_dtype=torch.float32)), tag
    gotr = ops.gemv_w8(xd, codes, scale, residual=rd)
    assert torch.equal(gotr.cpu(), (y32.to(torch.bfloat16).float() + res.float()).to(torch.bfloat16)), tag
    assert torch.equal(gotr, ops.gemv(xd, wd, residual=rd)), tag
    assert torch.equal(ops.gemv_w8(xd, codes, scale, residual=rd), gotr), "a second launch gives the same bits"


@pytest.mark.parametrize("M,N,K", [(1, 768, 512), (3, 1000, 1024), (2, 256, 320), (6, 192, 640)])
def test_shared_form_is_exact_on_grid_operands(dev, M, N, K):
    """One to six rows against one matrix: a step is 1024 elements of K, so K = 512 / 320 / 640 are a single ragged step, N = 1000 is ragged over
    a workgroup's sixteen rows, M = 6 is two passes."""
    _exact_shared(dev, torch.Generator().manual_seed(73 + M), M, N, K)


@pytest.mark.parametrize("N,K", [(4096, 4096), (4096, 11008), (1000, 4112)])
def test_ksplit_route_is_exact_on_grid_operands(dev, N, K):
    """N <= 4096, K >= 4096, one row: sixteen waves per sixteen rows, K split four ways (K = 11008: 10.75 steps; K = 4112: one lane's
    worth past four steps)."""
    _exact_shared(dev, torch.Generator().manual_seed(79), 1, N, K)


@pytest.mark.parametrize("E,N,K,M,idx,keep", [(3, 256, 512, 4, (2, 0, 1, 2), (0, 3, -1, 1)), (2, 4096, 11008, 3, (1, 0, 1), (0, -1, 1))])
def test_indexed_form_is_exact_on_grid_operands(dev, E, N, K, M, idx, keep):
    """The expert form (the wave-per-four-rows kernel at K = 512, the K-split one at 4096 x 11008): row m streams expert idx[m]'s codes and
    scales; combine weight on the bf16-rounded output, then the residual; a dropped row keeps its residual bits exactly."""
    from medplib_amd import ops
    g = torch.Generator().manual_seed(83)
    w, c, e = _grid(g, E, N, K)
    x, res = _ints(g, M, K), _bf(torch.randn(M, N, generator=g))
    rs = torch.tensor([0.7, 0.9, 0.55, 0.6][:M])
    idx_t, keep_t = torch.tensor(idx, dtype=torch.int32), torch.tensor(keep, dtype=torch.int32)
    rows = []
    for m in range(M):
        y32 = (x[m].double() @ w[idx[m]].double().T).float()
        rows.append(res[m] if keep[m] < 0 else (rs[m] * y32.to(torch.bfloat16).float() + res[m].float()).to(torch.bfloat16))
    ref = torch.stack(rows)
    wd = w.to(dev)
    codes, scale = ops.quantize_rows_w8(wd)
    kw = dict(residual=res.to(dev), w_index=idx_t.to(dev), row_scale=rs.to(dev), row_keep=keep_t.to(dev))
    got = ops.gemv_w8(x.to(dev), codes, scale, **kw)
    assert torch.equal(got.cpu(), ref)
    dropped = keep.index(-1)
    assert torch.equal(got[dropped].cpu(), res[dropped]), "a capacity-dropped row keeps the residual stream exactly"
    assert torch.equal(got, ops.gemv(x.to(dev), wd, **kw))
    assert torch.equal(ops.gemv_w8(x.to(dev), codes, scale, **kw), got), "a second launch gives the same bits"


def _dequant(codes, scale):
    return codes.float().cpu() * scale.cpu().unsqueeze(-1)


def test_random_operands_within_the_bf16_kernels_tolerances(dev):
    """Random x and W: the reference is fp32 x @ (code * scale)^T through the reference epilogue, so the quantisation error is on both sides
    and the kernel owes its own rounding only — at mp_gemv_bf16's tolerances."""
    from medplib_amd import ops
    g = torch.Generator().manual_seed(89)
    for M, N, K in ((1, 768, 512), (3, 1000, 1024), (2, 256, 320), (6, 192, 640), (1, 4096, 4096), (1, 1000, 4112)):
        x = _bf(torch.randn(M, K, generator=g)); w = _bf(torch.randn(N, K, generator=g) * 0.05); res = _bf(torch.randn(M, N, generator=g))
        codes, scale = ops.quantize_rows_w8(w.to(dev))
        ref = O.linear(x.float(), _dequant(codes, scale))
        _report(f"gemv_w8 {M}x{N}x{K}", ops.gemv_w8(x.to(dev), codes, scale), ref, rtol=2 * BF16_EPS, atol=1e-3 * math.sqrt(K))
        _report(f"gemv_w8 f32 out {M}x{N}x{K}", ops.gemv_w8(x.to(dev), codes, scale, out_dtype=torch.float32), ref, rtol=1e-4, atol=2e-3)
        _report(f"gemv_w8 residual {M}x{N}x{K}", ops.gemv_w8(x.to(dev), codes, scale, residual=res.to(dev)),
                ref.to(torch.bfloat16).float() + res.float(), rtol=2 * BF16_EPS, atol=2e-2)
    # SwiGLU pairing over the interleaved gate|up rows (a per-row scale is indifferent to the interleave)
    M, ff, K = 2, 320, 1024
    x = _bf(torch.randn(M, K, generator=g)).to(dev)
    wg = _bf(torch.randn(ff, K, generator=g) * 0.1).to(dev); wu = _bf(torch.randn(ff, K, generator=g) * 0.1).to(dev)
    (cg, sg), (cu, su) = ops.quantize_rows_w8(wg), ops.quantize_rows_w8(wu)
    codes, scale = ops.quantize_rows_w8(ops.swiglu_interleave(wg, wu))
    ref = O.swiglu(O.linear(x.float().cpu(), _dequant(cg, sg)), O.linear(x.float().cpu(), _dequant(cu, su)))
    _report("gemv_w8 swiglu pair", ops.gemv_w8(x, codes, scale, act=ops.ACT_SWIGLU_PAIR), ref, rtol=3 * BF16_EPS, atol=2e-2)
    # the indexed SwiGLU at E = 2, then the row_scale form on its output's shape
    E, M = 2, 3
    wg = _bf(torch.randn(E, ff, K, generator=g) * 0.1).to(dev); wu = _bf(torch.randn(E, ff, K, generator=g) * 0.1).to(dev)
    wi = torch.stack([ops.swiglu_interleave(wg[e], wu[e]) for e in range(E)])
    codes, scale = ops.quantize_rows_w8(wi)
    x = _bf(torch.randn(M, K, generator=g)).to(dev)
    idx = torch.tensor([1, 0, 1], dtype=torch.int32)
    (cg, sg), (cu, su) = ops.quantize_rows_w8(wg), ops.quantize_rows_w8(wu)
    dg, du = _dequant(cg, sg), _dequant(cu, su)
    ref = torch.stack([O.swiglu(O.linear(x[m:m + 1].float().cpu(), dg[idx[m]]), O.linear(x[m:m + 1].float().cpu(), du[idx[m]]))[0] for m in range(M)])
    _report("gemv_w8 indexed swiglu", ops.gemv_w8(x, codes, scale, act=ops.ACT_SWIGLU_PAIR, w_index=idx.to(dev)), ref, rtol=3 * BF16_EPS, atol=2e-2)
    N, K = 256, 512
    x = _bf(torch.randn(M, K, generator=g)); w = _bf(torch.randn(E, N, K, generator=g) * 0.05); res = _bf(torch.randn(M, N, generator=g))
    rs, keep = torch.tensor([0.7, 0.9, 0.55]), torch.tensor([0, 2, 1], dtype=torch.int32)
    codes, scale = ops.quantize_rows_w8(w.to(dev))
    dq = _dequant(codes, scale)
    ref = torch.stack([res[m].float() + rs[m] * (x[m].float() @ dq[idx[m]].t()).to(torch.bfloat16).float() for m in range(M)])
    got = ops.gemv_w8(x.to(dev), codes, scale, residual=res.to(dev), w_index=idx.to(dev), row_scale=rs.to(dev), row_keep=keep.to(dev))
    _report("gemv_w8 experts row_scale", got, ref, rtol=3 * BF16_EPS, atol=2e-2)
