"""Kernel-level parity of the fp32 tail (small_ops_f32.hip, sgemm_f32.hip): LayerNorm and softmax forward and backward, activations,
colsum, add, scale, gathers, the ConvT pixel shuffle and sgemm.  Float64 references with bounds derived from the kernels' operation
counts (beside the helpers in kernel_parity.py); equal bits wherever the inputs make the operation exact (integer-valued operands for
sums and products, arange payloads for data movement); outputs through strided views keep a canary around them.
Record: profiles/row_kernel_parity_tests.md."""
import pytest
import torch
import torch.nn.functional as F

from kernel_parity import (CANARY, COLSUM_COLS, COLSUM_ROWS, U32, ULP2, assert_bits, canary_intact, canary_view, gelu_grad_ref, gelu_ref,
                           gen, int_values, layernorm_bwd_ref, layernorm_ref, ln_f32_depth, offset_rows_f32, ratio_check, sgemm_cases,
                           sgemm_operands, softmax_bwd_ref, softmax_case, softmax_ref)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------- LayerNorm
def _ln_inputs(rows, dim, offset):
    g = gen(rows * 1000 + dim)
    x = offset_rows_f32(rows, dim, rows + dim) if offset else torch.randn(rows, dim, generator=g) * 2 + torch.randn(rows, 1, generator=g)
    return x, 1 + 0.5 * torch.randn(dim, generator=g), torch.randn(dim, generator=g), torch.randn(rows, dim, generator=g)


@pytest.mark.parametrize("dim", [1, 7, 63, 64, 65, 256, 1000])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 17])
@pytest.mark.parametrize("offset", [False, True])
def test_layernorm_f32_fwd_bwd(dev, dim, rows, offset):
    """y, mean and rstd against float64; dx against float64 from the kernel's own mean / rstd; offset = rows with mean 1e3 and spread
    1e-2 (a one-pass variance has no digits left there).  dim = 1: y == b to the bit."""
    from medplib_amd import ops
    x, w, b, dy = _ln_inputs(rows, dim, offset)
    eps = 1e-6
    r = layernorm_ref(x, w, b, eps, ln_f32_depth(dim), e_root=2 * ULP2)
    y, mean, rstd = ops.layernorm_fwd_f32(x.to(dev), w.to(dev), b.to(dev), eps)
    torch.cuda.synchronize()
    tag = f"dim={dim} rows={rows} offset={offset}"
    ratio_check(f"ln_f32 y {tag}", y, r["y"], r["E"])
    ratio_check(f"ln_f32 mean {tag}", mean, r["mean"], r["dm"])
    ratio_check(f"ln_f32 rstd {tag}", rstd, r["rstd"], r["rstd"] * r["e_rs"])
    if dim == 1:
        assert_bits("ln_f32 dim=1: y == b", y, b.expand(rows, 1))
    rb = layernorm_bwd_ref(dy, x, w, mean.cpu(), rstd.cpu())
    dx = ops.layernorm_bwd_f32(dy.to(dev), x.to(dev), w.to(dev), mean, rstd, None, None)
    ratio_check(f"ln_f32 dx {tag}", dx, rb["dx"], rb["dx_bound"])


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("dim", [7, 65])
def test_layernorm_f32_dw_db(dev, rows, dim):
    """dw / db accumulate into NON-ZERO preset buffers (rows striped over 16 waves: 1, 15, 16, 17, 33 rows leave the stripes uneven);
    only dw given, only db given; two launches give equal bits."""
    from medplib_amd import ops
    x, w, b, dy = _ln_inputs(rows, dim, False)
    _, mean, rstd = ops.layernorm_fwd_f32(x.to(dev), w.to(dev), b.to(dev), 1e-6)
    rb = layernorm_bwd_ref(dy, x, w, mean.cpu(), rstd.cpu())
    pw, pb = torch.randn(dim, generator=gen(rows)) * 3, torch.randn(dim, generator=gen(rows + 1)) * 3
    xd, wd, dyd = x.to(dev), w.to(dev), dy.to(dev)

    def run(want_w, want_b):
        dw, db = pw.to(dev), pb.to(dev)
        dx = ops.layernorm_bwd_f32(dyd, xd, wd, mean, rstd, dw if want_w else None, db if want_b else None)
        torch.cuda.synchronize()
        return dx.cpu(), dw.cpu(), db.cpu()
    dx, dw, db = run(True, True)
    tag = f"rows={rows} dim={dim}"
    ratio_check(f"ln_f32 dx {tag}", dx, rb["dx"], rb["dx_bound"])
    ratio_check(f"ln_f32 dw += {tag}", dw, pw.double() + rb["dw"], rb["dw_bound"] + U32 * (pw.double().abs() + rb["dw"].abs()))
    ratio_check(f"ln_f32 db += {tag}", db, pb.double() + rb["db"], rb["db_bound"] + U32 * (pb.double().abs() + rb["db"].abs()))
    dx2, dw2, db2 = run(True, True)
    assert_bits("second launch dx", dx2, dx); assert_bits("second launch dw", dw2, dw); assert_bits("second launch db", db2, db)
    dx3, dw3, db3 = run(True, False)
    assert_bits("only dw: dw", dw3, dw); assert_bits("only dw: db untouched", db3, pb); assert_bits("only dw: dx", dx3, dx)
    dx4, dw4, db4 = run(False, True)
    assert_bits("only db: db", db4, db); assert_bits("only db: dw untouched", dw4, pw); assert_bits("only db: dx", dx4, dx)


# ------------------------------------------------------------------------------------------------------------------------ softmax
@pytest.mark.parametrize("cols", [1, 2, 7, 63, 64, 65, 256, 4096])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("scale", [1.0, 0.125])
def test_softmax_f32(dev, cols, rows, scale):
    from medplib_amd import ops
    for kind in ("random", "equal", "spread", "neginf"):
        x = softmax_case(kind, rows, cols, cols + rows)
        p, bound, c = softmax_ref(x, scale)
        got = ops.softmax_fwd_f32(x.to(dev), scale)
        torch.cuda.synchronize()
        tag = f"{kind} cols={cols} rows={rows} scale={scale}"
        ratio_check(f"softmax fwd {tag}", got, p, bound)
        gc = got.cpu()
        if kind == "equal":
            assert bool((gc == gc[:, :1]).all()), "equal entries must give equal outputs"
            dev1 = (gc.double().sum(-1) - 1).abs()
            assert bool((dev1 <= c + cols * U32).all()), f"row sums off by {float(dev1.max()):.3e}"
        if kind == "neginf":
            assert bool((gc[:, 1::2] == 0).all()), "-inf entries must give exact zeros"
        if kind == "spread" and cols > 1:
            assert bool((gc[:, -1] == 0).all())
        dp = torch.randn(rows, cols, generator=gen(cols))
        dx, dbound = softmax_bwd_ref(gc, dp, scale)
        ratio_check(f"softmax bwd {tag}", ops.softmax_bwd_f32(got, dp.to(dev), scale), dx, dbound)


# -------------------------------------------------------------------------------------------------------------------- activations
def _act_grid(n):
    x = torch.cat([torch.linspace(-10, 10, max(n - 2, 0)), torch.tensor([0.0, -0.0])])[-n:] if n > 2 else torch.tensor([0.0, -0.0, 1.5])[:n]
    return x.float().contiguous()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
def test_activations_f32(dev, n):
    from medplib_amd import ops
    x = _act_grid(n)
    assert x.numel() == n
    dy = torch.randn(n, generator=gen(n))
    xd, dyd = x.to(dev), dy.to(dev)
    assert_bits(f"relu fwd n={n}", ops.act_fwd_f32(xd, ops.SACT_RELU).cpu() + 0.0, torch.relu(x) + 0.0)      # + 0.0: fmaxf(-0, 0) may be either zero
    assert_bits(f"relu bwd n={n}", ops.act_bwd_f32(dyd, xd, ops.SACT_RELU), torch.where(x > 0, dy, torch.zeros_like(dy)))
    y, yb = gelu_ref(x)
    ratio_check(f"gelu fwd n={n}", ops.act_fwd_f32(xd, ops.SACT_GELU), y, yb)
    gy, gb = gelu_grad_ref(dy, x)
    ratio_check(f"gelu bwd n={n}", ops.act_bwd_f32(dyd, xd, ops.SACT_GELU), gy, gb)
    # form 3: x holds the sigmoid OUTPUT s; dx = dy s (1 - s): the difference and two products, 3 roundings (4 U32 asserted)
    s = torch.sigmoid(torch.linspace(-12, 12, n)).float() if n > 1 else torch.tensor([0.3])
    ref = dy.double() * s.double() * (1 - s.double())
    ratio_check(f"act_bwd form 3 n={n}", ops.act_bwd_f32(dyd, s.to(dev), 3), ref, 4 * U32 * ref.abs())


# ------------------------------------------------------------------------------------------------------- colsum, add, scale
@pytest.mark.parametrize("rows", COLSUM_ROWS)
def test_colsum_exact(dev, rows):
    """Integer-valued input: every partial sum is exact, so any order gives the float64 sum bit for bit; rows walk the edges of the
    4-accumulator loop (r + 48 < rows) and of the 16-row remainder loop.  rows = 0: zeros, or the preset unchanged under accumulate."""
    from medplib_amd import ops
    for cols in COLSUM_COLS:
        x = int_values((rows, cols), rows * 131 + cols)
        ref = x.double().sum(0)
        whole, out = canary_view(1, cols, cols + 8, torch.float32, dev)
        ops.colsum_f32(x.to(dev), out=out[0])
        assert_bits(f"colsum rows={rows} cols={cols}", ops.colsum_f32(x.to(dev)), ref.float())
        assert_bits("colsum into a view", out[0], ref.float())
        canary_intact("colsum out", whole, 1, cols, cols + 8)
        preset = int_values((cols,), cols, lim=1000)
        acc = preset.to(dev)
        ops.colsum_f32(x.to(dev), out=acc, accumulate=True)
        assert_bits(f"colsum accumulate rows={rows} cols={cols}", acc, (preset.double() + ref).float())


@pytest.mark.parametrize("period", [1, 7, 0])
def test_add_f32(dev, period):
    from medplib_amd import ops
    n = 7 * 257
    period = period or n
    a, b = torch.randn(n, generator=gen(period)), torch.randn(period, generator=gen(period + 1))
    assert_bits(f"add_f32 period={period}", ops.add_f32(a.to(dev), b.to(dev)), a + b.repeat(n // period))


@pytest.mark.parametrize("n", [1, 256, 257])
def test_scale_f32(dev, n):
    from medplib_amd import ops
    x = torch.randn(n + 2, generator=gen(n))
    buf = x.to(dev)
    ops.scale_f32_(buf[1:1 + n], 0.3)
    ref = x.clone()
    ref[1:1 + n] = x[1:1 + n] * torch.tensor(0.3, dtype=torch.float32)
    assert_bits(f"scale_f32_ n={n}", buf, ref)


# ------------------------------------------------------------------------------------------------------------------------ gathers
@pytest.mark.parametrize("dim", [1, 5, 64, 257])
def test_gathers_exact(dev, dim):
    """arange-distinct payloads; repeated indices, the first and the last row; the bf16 source as a view with a row stride."""
    from medplib_amd import ops
    n = 23
    idx = torch.tensor([n - 1, 0, 7, 7, 0, n - 1, 3, 7], dtype=torch.int64)
    src = (torch.arange(n * dim, dtype=torch.int32) + 0x0100).to(torch.int16).view(torch.bfloat16).view(n, dim)      # distinct finite patterns
    wide = torch.full((n, dim + 3), CANARY, dtype=torch.bfloat16, device=dev)
    wide[:, :dim] = src.to(dev)
    for s in (src.to(dev), wide[:, :dim]):
        assert_bits(f"gather bf16->f32 dim={dim} ld={s.stride(0)}", ops.gather_rows_bf16_to_f32(s, idx.to(dev)), src[idx].float())
    f = torch.arange(n * dim * 2).float().view(n, dim, 2)
    assert_bits(f"gather f32 dim={dim}", ops.gather_rows_f32(f.to(dev), idx.to(dev)), f[idx])


# -------------------------------------------------------------------------------------------------------------------- ConvT shuffle
@pytest.mark.parametrize("B,h,w,Co", [(3, 2, 5, 3), (1, 16, 64, 32), (2, 1, 1, 1)])
def test_convt_shuffle_exact(dev, B, h, w, Co):
    """G = arange: forward equals F.conv_transpose2d(k=2, s=2) with a one-hot weight (which makes the convolution the permutation
    G[pixel, co*4 + kh*2 + kw] -> Y[b, 2i+kh, 2j+kw, co], every sum exact) plus bias, bit for bit; h != w; bwd(fwd(G, None)) == G."""
    from medplib_amd import ops
    n = B * h * w * Co * 4
    G = torch.arange(n).float().view(B * h * w, Co * 4)
    bias = torch.arange(Co).float() * 0.5 - 3
    W = torch.eye(Co * 4).view(Co * 4, Co, 2, 2)
    conv = F.conv_transpose2d(G.view(B, h, w, Co * 4).permute(0, 3, 1, 2), W, None, stride=2).permute(0, 2, 3, 1).contiguous()
    perm = G.view(B, h, w, Co, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * h, 2 * w, Co)
    assert torch.equal(conv, perm) and n < 2 ** 24
    Gd = G.to(dev)
    assert_bits(f"convt fwd + bias {B, h, w, Co}", ops.convt2x2_shuffle_fwd(Gd, bias.to(dev), B, h, w, Co), conv + bias)
    Y = ops.convt2x2_shuffle_fwd(Gd, None, B, h, w, Co)
    assert_bits("convt fwd, bias=None", Y, conv)
    assert_bits("convt bwd(fwd(G)) == G", ops.convt2x2_shuffle_bwd(Y, B, h, w, Co), G)


# -------------------------------------------------------------------------------------------------------------------------- sgemm
def _flags(form):
    return {"trans_a": form == "TN", "trans_b": form == "NT"}


@pytest.mark.parametrize("form", ["NN", "NT", "TN"])
def test_sgemm_exact_edges(dev, form):
    """Integer-valued operands: the fp32 result equals float64 bit for bit at every ragged edge (63 / 64 / 65 / 129 in M and N, 15 ..
    130 in K, the K = 63 / 64 pair on either side of the 16-deep / 64-deep kernel switch)."""
    from medplib_amd import ops
    for f, M, N, K in sgemm_cases():
        if f != form:
            continue
        a, b, ref = sgemm_operands(form, M, N, K, M * 7 + N * 3 + K)
        assert_bits(f"sgemm {form} {M}x{N}x{K}", ops.sgemm(a.to(dev), b.to(dev), **_flags(form)), ref.float())


@pytest.mark.parametrize("form,M,N,K", [("NN", 65, 63, 64), ("NT", 63, 129, 17), ("TN", 129, 65, 130)])
def test_sgemm_exact_epilogues(dev, form, M, N, K):
    """alpha / beta onto a preset C, beta = 0 onto NaN, bias + ReLU, out= as a view with ldc > N (canary): all exact in fp32 with
    integer operands (0.5 and 0.25 only move the exponent)."""
    from medplib_amd import ops
    a, b, ref = sgemm_operands(form, M, N, K, K)
    ad, bd = a.to(dev), b.to(dev)
    c0 = int_values((M, N), K + 5, lim=100)
    whole, out = canary_view(M, N, N + 5, torch.float32, dev)
    out.copy_(c0.to(dev))
    ops.sgemm(ad, bd, alpha=0.5, beta=0.25, out=out, **_flags(form))
    assert_bits("alpha=0.5 beta=0.25 into a strided view", out, (0.5 * ref + 0.25 * c0.double()).float())
    canary_intact("sgemm out", whole, M, N, N + 5)
    nan_c = torch.full((M, N), float("nan"), device=dev)
    ops.sgemm(ad, bd, beta=0.0, out=nan_c, **_flags(form))
    assert_bits("beta=0 onto NaN", nan_c, ref.float())
    bias = int_values((N,), K + 9, lim=50)
    assert_bits("bias + relu", ops.sgemm(ad, bd, bias=bias.to(dev), act=ops.SACT_RELU, **_flags(form)), torch.relu(ref + bias.double()).float())


def test_sgemm_sigmoid_and_gelu(dev):
    """Random data: v = a @ b + bias carries K fma roundings (K U32 sum|a||b|) and the bias add; sigmoid 1 / (1 + expf(-v)) has slope
    <= 1/4 and ULP2 for expf, ULP2 for the division, one addition; GELU: kernel_parity.gelu_ref with the input's error."""
    from medplib_amd import ops
    for form, M, N, K in (("NN", 65, 63, 64), ("NT", 63, 129, 17), ("TN", 129, 65, 130)):
        g = gen(K)
        a, b, bias = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g), torch.randn(N, generator=g)
        v = a.double() @ b.double() + bias.double()
        dv = (K + 1) * U32 * (a.double().abs() @ b.double().abs()) + U32 * v.abs()
        sa = a.t().contiguous() if form == "TN" else a
        sb = b.t().contiguous() if form == "NT" else b
        sg = torch.sigmoid(v)
        ratio_check(f"sgemm sigmoid {form}", ops.sgemm(sa.to(dev), sb.to(dev), bias=bias.to(dev), act=ops.SACT_SIGMOID, **_flags(form)), sg,
                    0.25 * dv + (2 * ULP2 + 2 * U32) * sg)
        y, yb = gelu_ref(v, dv=dv)
        ratio_check(f"sgemm gelu {form}", ops.sgemm(sa.to(dev), sb.to(dev), bias=bias.to(dev), act=ops.SACT_GELU, **_flags(form)), y, yb)


def test_sgemm_split_k_exact(dev):
    """Atomic split-K onto a preset C.  The parts are ceil(K / split_k) rounded up to the slab depth (16 below 64 per part, 64 from
    there): split_k = 4 at K = 130 gives 48, 48, 34; at K = 17 gives 16, 1 and two EMPTY parts; at K = 260 (64-deep) 128, 128, 4 and an
    empty one; split_k = 8 at K = 1000 seven parts of 128 and a short one of 104.  Then the wrapper's automatic deterministic split at
    a skinny K = 1024.  Integer operands: exact."""
    from medplib_amd import ops
    for form, M, N, K, sp in (("NN", 63, 65, 130, 4), ("NT", 5, 129, 130, 4), ("TN", 65, 64, 1000, 8), ("NN", 1, 63, 1000, 8),
                              ("NT", 65, 63, 17, 4), ("TN", 64, 65, 260, 4)):
        a, b, ref = sgemm_operands(form, M, N, K, K + sp)
        c0 = int_values((M, N), sp, lim=100)
        whole, out = canary_view(M, N, N + 3, torch.float32, dev)
        out.copy_(c0.to(dev))
        ops.sgemm(a.to(dev), b.to(dev), out=out, beta=1.0, split_k=sp, **_flags(form))
        assert_bits(f"sgemm split_k={sp} {form} {M}x{N}x{K}", out, (c0.double() + ref).float())
        canary_intact("split-K out", whole, M, N, N + 3)
    for form in ("NN", "NT", "TN"):
        a, b, ref = sgemm_operands(form, 6, 65, 1024, 11)
        bias = int_values((65,), 12, lim=50)
        assert_bits(f"sgemm automatic split {form}", ops.sgemm(a.to(dev), b.to(dev), **_flags(form)), ref.float())
        assert_bits(f"sgemm automatic split + bias + relu {form}", ops.sgemm(a.to(dev), b.to(dev), bias=bias.to(dev), act=ops.SACT_RELU, **_flags(form)),
                    torch.relu(ref + bias.double()).float())


def test_sgemm_strided_two_level_batch_exact(dev):
    """[B, H] batch through strided head views with ragged M = 65 and N = 63 (scores = q k^T, then probabilities @ v)."""
    from medplib_amd import ops
    B, H, Nq, Nk, d = 2, 3, 65, 63, 17
    q, k = int_values((B, Nq, H * d), 1), int_values((B, Nk, H * d), 2)
    qv = q.to(dev).view(B, Nq, H, d).permute(0, 2, 1, 3)
    kv = k.to(dev).view(B, Nk, H, d).permute(0, 2, 1, 3)
    ref = torch.einsum("bqhd,bkhd->bhqk", q.double().view(B, Nq, H, d), k.double().view(B, Nk, H, d))
    s = ops.sgemm(qv, kv, trans_b=True, alpha=0.5)
    assert_bits("batched NT scores", s, (0.5 * ref).float())
    o = ops.sgemm(s, kv)                                              # NN: [B,H,Nq,Nk] @ [B,H,Nk,d], |s| <= 64 * 17 / 2: partials < 2^24
    ref_o = torch.einsum("bhqk,bkhd->bhqd", 0.5 * ref, k.double().view(B, Nk, H, d))
    assert float((0.5 * ref).abs().max()) * 8 * Nk < 2 ** 24
    assert_bits("batched NN", o, ref_o.float())
