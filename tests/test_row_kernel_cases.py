"""CPU-only guard of the crafted inputs and references behind tests/test_gpu_row_kernels.py and tests/test_gpu_f32_tail_kernels.py:
the inputs are what those tests claim (ties, exact sums, underflowing terms, offset rows), and every float64 reference, evaluated
against a plain fp32 torch form of the same operation on the same inputs, stays inside the bound it is used with."""
import torch
import torch.nn.functional as F

from kernel_parity import (COLSUM_COLS, COLSUM_ROWS, LN_BF16_DEPTH, SGEMM_K, SGEMM_MN, ULP2, bf, bits, cast_tie_sweep, gelu_grad_ref, gelu_ref,
                           gen, int_values, layernorm_bf16_bound, layernorm_bwd_ref, layernorm_ref, ln_f32_depth, offset_rows_bf16,
                           offset_rows_f32, ratio_check, rmsnorm_ref, rope_ref, sgemm_cases, sgemm_operands, softmax_bwd_ref, softmax_case,
                           softmax_ref, swiglu_ref, swiglu_sweep)


def test_cast_sweep_holds_a_tie_and_its_neighbours_at_every_exponent():
    s = cast_tie_sweep()
    b = s.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    ties = b[(b & 0xFFFF) == 0x8000]
    ties = ties[((ties >> 23) & 0xFF) != 0xFF]
    assert bool((torch.isin(ties - 1, b) & torch.isin(ties + 1, b)).all())
    key = (ties >> 23) & 0x1FF                                             # sign and exponent field
    for parity in (0, 1):                                                  # a tie above an even and above an odd pattern
        assert set(key[((ties >> 16) & 1) == parity].tolist()) == set(range(255)) | set(range(256, 511)), parity
    # round-to-nearest-even and round-half-up differ on exactly the ties above an even pattern: the sweep tells them apart
    rne = bits(s.bfloat16()).to(torch.int64) & 0xFFFF
    half_up = ((b + 0x8000) >> 16) & 0xFFFF
    fin = torch.isfinite(s)
    assert int((rne != half_up)[fin].sum()) > 30000
    # the eight ties at the end alternate: rounds down (even pattern below), rounds up
    last = b[-8:]
    assert bool(((last & 0xFFFF) == 0x8000).all()) and [(int(v) >> 16) & 1 for v in last] == [0, 1] * 4
    assert {s.numel() % 4, (s.numel() - 1) % 4, (s.numel() - 2) % 4, (s.numel() - 3) % 4} == {0, 1, 2, 3}
    for special in (float("inf"), float("-inf"), 3.4028234663852886e38):
        assert bool((s == special).any())
    assert bool(torch.isnan(s).sum() >= 4) and bool(((s != 0) & (s.abs() < 2.0 ** -126)).any())


def test_integer_operands_keep_every_partial_sum_exact():
    cases = sgemm_cases()
    for form in ("NN", "NT", "TN"):
        assert {K for f, M, N, K in cases if f == form} == set(SGEMM_K)
        assert {M for f, M, N, K in cases if f == form} == set(SGEMM_MN) == {N for f, M, N, K in cases if f == form}
        assert {(65, 65, 63), (65, 65, 64)} <= {(M, N, K) for f, M, N, K in cases if f == form}
    for form, M, N, K in cases + [("NN", 6, 65, 1024), ("TN", 65, 64, 1000), ("NN", 63, 65, 130)]:
        a, b, ref = sgemm_operands(form, M, N, K, 1)
        am = a.t() if form == "TN" else a
        bm = b.t() if form == "NT" else b
        assert am.shape == (M, K) and bm.shape == (K, N)
        assert float(a.abs().max()) <= 8 and float(b.abs().max()) <= 8 and bool((a == a.round()).all())
        worst = float((am.double().abs() @ bm.double().abs()).max())           # the largest sum of |products|: bounds every partial sum
        assert worst + 100 < 2 ** 24                                           # + the preset C (|c0| <= 100)
        assert torch.equal(ref.float().double(), ref)
    for rows in COLSUM_ROWS:
        for cols in COLSUM_COLS:
            x = int_values((rows, cols), rows * 131 + cols)
            assert float(x.abs().sum(0).max()) + 1000 < 2 ** 24 if rows else x.numel() == 0


def test_softmax_cases_hold_what_they_claim():
    for cols in (2, 7, 63, 64, 65, 256, 4096):
        for scale in (1.0, 0.125):
            x = softmax_case("spread", 5, cols, cols) * scale
            gap = x.double() - x.double().amax(-1, keepdim=True)
            assert bool((gap < -104).any(-1).all())                            # exp below 2^-149: the term is zero in fp32
            assert bool((gap == 0).any(-1).all())
        n = softmax_case("neginf", 5, cols, cols)
        assert bool(torch.isinf(n[:, 1::2]).all() and torch.isfinite(n[:, 0::2]).all())
        e = softmax_case("equal", 5, cols, cols)
        assert bool((e == e[:, :1]).all()) and float(e[0, 0]) != float(e[1, 0])


def test_offset_rows_have_the_stated_mean_to_spread_ratio():
    for dim in (8, 520, 768, 2048, 2056, 8192):
        x = offset_rows_bf16(5, dim, dim).double()                             # after the bf16 rounding
        assert set(x.unique().tolist()) <= {99.5, 100.0, 100.5}
        assert bool((x.mean(-1).abs() / x.std(-1, unbiased=False) > 200).all()), dim
        assert float(x.abs().sum(-1).max()) < 2 ** 23 * 0.5 * 2                # multiples of 0.5 below 2^24 * 0.5: every partial sum exact
    for dim in (7, 63, 64, 65, 256, 1000):
        x = offset_rows_f32(5, dim, 5 + dim).double()
        r = x.mean(-1).abs() / x.std(-1, unbiased=False)
        assert bool((r > 5e4).all() and (r < 4e5).all()), (dim, r)


def test_references_stay_inside_their_own_bounds():
    """Each float64 reference against fp32 torch on the same inputs, with the bound the GPU test uses."""
    g = gen(1)
    # RMSNorm, HF order in fp32
    for dim in (8, 264, 4104):
        x = (torch.randn(5, dim, generator=g) * 2).bfloat16(); w = 1 + 0.5 * torch.randn(dim, generator=g)
        ref, bound = rmsnorm_ref(x, w, 1e-5)
        xf = x.float()
        t = bf(xf * torch.rsqrt((xf * xf).mean(-1, keepdim=True) + 1e-5))
        ratio_check(f"rmsnorm fp32 torch dim={dim}", bf(w * t), ref, bound)
    # LayerNorm bf16 (ordinary and offset rows) and fp32
    for dim in (8, 520, 2056):
        w = 1 + 0.5 * torch.randn(dim, generator=g); b = torch.randn(dim, generator=g)
        for x, exact in (((torch.randn(4, dim, generator=g) * 2 + 1).bfloat16(), False), (offset_rows_bf16(4, dim, dim), True)):
            r = layernorm_ref(x, w, b, 1e-5, LN_BF16_DEPTH, sum_exact=exact)
            got = bf(F.layer_norm(x.double(), (dim,), w.double(), b.double(), 1e-5).float())     # the exact value, rounded once
            ratio_check(f"layernorm bf16 dim={dim} exact_sums={exact}", got, r["y"], layernorm_bf16_bound(r))
    for dim in (1, 7, 65, 1000):
        for x in (torch.randn(5, dim, generator=g) * 2 + 1, offset_rows_f32(5, dim, dim)):
            x = x.clone().requires_grad_(True)
            w = (1 + 0.5 * torch.randn(dim, generator=g)).requires_grad_(True); b = torch.randn(dim, generator=g).requires_grad_(True)
            dy = torch.randn(5, dim, generator=g)
            r = layernorm_ref(x.detach(), w.detach(), b.detach(), 1e-6, ln_f32_depth(dim), e_root=2 * ULP2)
            y64 = F.layer_norm(x.detach().double(), (dim,), w.detach().double(), b.detach().double(), 1e-6)
            ratio_check(f"layernorm f32 dim={dim}", y64.float(), r["y"], r["E"])
            # backward: float64 autograd against the restated formula fed with fp32-rounded statistics
            x64 = x.detach().double().requires_grad_(True); w64 = w.detach().double().requires_grad_(True); b64 = b.detach().double().requires_grad_(True)
            F.layer_norm(x64, (dim,), w64, b64, 1e-6).backward(dy.double())
            rb = layernorm_bwd_ref(dy, x.detach(), w.detach(), r["mean"].float(), r["rstd"].float())
            # the statistics' own fp32 rounding moves xhat by U32 (|mean| rstd + |xhat|): the restated dx may differ from autograd by that much
            slack = 2.0 ** -24 * (r["mean"].abs() * r["rstd"])[:, None] * (rb["dx"].abs() + (dy.double() * w.detach().double()).abs().mean(-1, keepdim=True) * r["rstd"][:, None]) * 4
            ratio_check(f"layernorm f32 dx dim={dim}", x64.grad, rb["dx"], rb["dx_bound"] + slack + 1e-30)
    # softmax
    for kind in ("random", "equal", "spread", "neginf"):
        for scale in (1.0, 0.125):
            x = softmax_case(kind, 5, 65, 3)
            p, bound, c = softmax_ref(x, scale)
            got = torch.softmax(x * scale, -1)
            ratio_check(f"softmax fp32 torch {kind}", got, p, bound)
            dp = torch.randn(5, 65, generator=g)
            dx, db = softmax_bwd_ref(got, dp, scale)
            s = (got * dp).sum(-1, keepdim=True)
            ratio_check(f"softmax bwd fp32 torch {kind}", scale * got * (dp - s), dx, db)
    # GELU and its derivative
    x = torch.cat([torch.linspace(-10, 10, 4001), torch.tensor([0.0, -0.0])]).float()
    dy = torch.randn(x.numel(), generator=g)
    y, yb = gelu_ref(x)
    k = torch.tensor(0.7071067811865476, dtype=torch.float32)
    cdf = 0.5 * (1 + torch.erf(x * k))                                         # the kernel's own formula, term by term in fp32
    ratio_check("gelu fp32 torch", 0.5 * x * (1 + torch.erf(x * k)), y, yb)
    gy, gb = gelu_grad_ref(dy, x)
    ratio_check("gelu grad fp32 torch", dy * (cdf + x * (torch.tensor(0.3989422804014327, dtype=torch.float32) * torch.exp(-0.5 * x * x))), gy, gb)
    # SwiGLU: fp32 torch over the sweep, one bf16 ulp + the floor
    gu, n = swiglu_sweep()
    Fh = gu.shape[1] // 2
    gv, uv = gu[:, :Fh].float(), gu[:, Fh:].float()
    ref, ulp, floor = swiglu_ref(gv, uv)
    ratio_check("swiglu fp32 torch", bf(gv * torch.sigmoid(gv) * uv), ref, ulp + floor)
    assert n == int((torch.isfinite(gu[0, :Fh].float()) & (gu[0, :Fh].float() != 0)).sum()) + 2 and float(gv.min()) == -100 and float(gv.max()) == 100
    # RoPE
    lo, hi = torch.randn(37, 64, generator=g).bfloat16().float(), torch.randn(37, 64, generator=g).bfloat16().float()
    ang = torch.rand(37, 64, generator=g) * 6.283
    c, s = torch.cos(ang), torch.sin(ang)
    rl, rh, bl, bh = rope_ref(lo.double(), hi.double(), c.double(), s.double())
    ratio_check("rope lo fp32 torch", bf(lo * c - hi * s), rl, bl)
    ratio_check("rope hi fp32 torch", bf(hi * c + lo * s), rh, bh)
