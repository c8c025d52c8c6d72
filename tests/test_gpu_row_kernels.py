"""Kernel-level parity of the bf16 trunk's row and elementwise kernels (norm_elementwise.hip): RMSNorm, both LayerNorm kernels, RoPE,
decode RoPE + append, SwiGLU, the two casts, add_rows, add3, advance_ints.  Each kernel against float64 torch on the same bf16 / fp32
input values with a bound derived from its operation count (beside the helpers in kernel_parity.py), equal bits wherever the operation
is exact, at the sizes where the kernels change path (the 2048 / 2056 LayerNorm switch, partly filled chunks, partial last blocks),
through strided views whose surroundings hold a canary.  Record: profiles/row_kernel_parity_tests.md."""
import pytest
import torch

from kernel_parity import (CANARY, LN_BF16_DEPTH, U32, U_BF16, assert_bits, assert_bits_nan, bf16_ulp, bits, canary_intact, canary_view,
                           cast_tie_sweep, gen, layernorm_bf16_bound, layernorm_ref, offset_rows_bf16, ratio_check, rmsnorm_ref, rope_ref,
                           strided_in, swiglu_ref, swiglu_sweep)

pytestmark = pytest.mark.gpu


def _rows_x(rows, dim, seed):
    g = gen(seed)
    return (torch.randn(rows, dim, generator=g) * (0.5 + torch.rand(rows, 1, generator=g) * 3)).bfloat16()


# ------------------------------------------------------------------------------------------------------------------------ RMSNorm
@pytest.mark.parametrize("dim", [8, 264, 2048, 2056, 4096, 4104, 8192])
@pytest.mark.parametrize("rows", [1, 5])
def test_rmsnorm(dev, dim, rows):
    """Contiguous and strided (ld = dim + 8 in, dim + 24 out) give the same bits; both inside the derived bound; canary intact."""
    from medplib_amd import ops
    x = _rows_x(rows, dim, dim + rows)
    w = 1 + 0.5 * torch.randn(dim, generator=gen(dim))
    eps = 1e-5
    ref, bound = rmsnorm_ref(x, w, eps)
    wd = w.to(dev)
    got = ops.rmsnorm(x.to(dev), wd, eps)
    whole, out = canary_view(rows, dim, dim + 24, torch.bfloat16, dev)
    got_s = ops.rmsnorm(strided_in(x, dim + 8, dev), wd, eps, out=out)
    torch.cuda.synchronize()
    ratio_check(f"rmsnorm dim={dim} rows={rows}", got, ref, bound)
    assert_bits("rmsnorm strided == contiguous", got_s, got)
    canary_intact("rmsnorm out", whole, rows, dim, dim + 24)


def test_rmsnorm_zero_and_tiny_rows(dev):
    """An all-zero row gives exact zeros; a row of 1e-20-scale values, where eps is the whole denominator, stays inside the bound."""
    from medplib_amd import ops
    dim = 264
    x = _rows_x(3, dim, 7)
    x[0] = 0
    x[1] = (1e-20 * torch.randn(dim, generator=gen(8))).bfloat16()
    w = 1 + 0.5 * torch.randn(dim, generator=gen(9))
    for eps in (1e-5, 1e-6):
        ref, bound = rmsnorm_ref(x, w, eps)
        got = ops.rmsnorm(x.to(dev), w.to(dev), eps).cpu()
        assert bool((got[0].float() == 0).all()), "all-zero row"
        assert float(ref[1].abs().max()) > 1e-19                       # eps dominates: the row is scaled by 1 / sqrt(eps), not normalised
        ratio_check(f"rmsnorm zero/tiny rows eps={eps}", got, ref, bound)


@pytest.mark.parametrize("dim", [8200, 12])
def test_rmsnorm_unsupported_dim_raises(dev, dim):
    from medplib_amd import ops
    from medplib_amd._lib import MedplibError
    x = torch.zeros(2, dim, dtype=torch.bfloat16, device=dev)
    out = torch.full((2, dim), CANARY, dtype=torch.bfloat16, device=dev)
    with pytest.raises(MedplibError, match="unsupported"):
        ops.rmsnorm(x, torch.ones(dim, device=dev), 1e-5, out=out)
    torch.cuda.synchronize()
    assert_bits("output after the refused call", out, torch.full((2, dim), CANARY, dtype=torch.bfloat16))


# ---------------------------------------------------------------------------------------------------------------------- LayerNorm
LN_DIMS = [8, 520, 768, 2048, 2056, 8192]        # wave kernel up to 2048 (520: a partly filled second chunk), block kernel beyond


@pytest.mark.parametrize("dim", LN_DIMS)
@pytest.mark.parametrize("rows", [1, 4, 5, 7])
def test_layernorm(dev, dim, rows):
    """b given and b=None, contiguous and strided; the wave kernel packs four rows per block, so 1, 4, 5 and 7 rows leave 3, 0, 3 and 1
    waves of the last block without a row."""
    from medplib_amd import ops
    x = (_rows_x(rows, dim, 3 * dim + rows).float() + torch.randn(rows, 1, generator=gen(dim))).bfloat16()
    w = 1 + 0.5 * torch.randn(dim, generator=gen(dim + 1))
    b = torch.randn(dim, generator=gen(dim + 2))
    eps = 1e-5
    for bias in (b, None):
        r = layernorm_ref(x, w, bias, eps, LN_BF16_DEPTH)
        bd = None if bias is None else bias.to(dev)
        wd = w.to(dev)
        got = ops.layernorm(x.to(dev), wd, bd, eps)
        whole, out = canary_view(rows, dim, dim + 16, torch.bfloat16, dev)
        got_s = ops.layernorm(strided_in(x, dim + 8, dev), wd, bd, eps, out=out)
        torch.cuda.synchronize()
        ratio_check(f"layernorm dim={dim} rows={rows} b={'yes' if bias is not None else 'none'}", got, r["y"], layernorm_bf16_bound(r))
        assert_bits("layernorm strided == contiguous", got_s, got)
        canary_intact("layernorm out", whole, rows, dim, dim + 16)


@pytest.mark.parametrize("dim", LN_DIMS)
def test_layernorm_offset_and_constant_rows(dev, dim):
    """Rows with mean 100 and a spread of one bf16 step: the sums are exact, so the bound is the store's rounding plus a few fp32
    roundings -- a one-pass variance (E[x^2] - mean^2 at 1e4) loses the 0.17 variance's digits and fails it.  A constant row: x - mean
    is exactly 0, the output is bf16(b) to the bit (zero without b)."""
    from medplib_amd import ops
    rows = 5
    x = offset_rows_bf16(rows, dim, dim)
    x[2] = 3.0
    w = 1 + 0.5 * torch.randn(dim, generator=gen(dim + 1))
    b = torch.randn(dim, generator=gen(dim + 2))
    eps = 1e-5
    for bias in (b, None):
        r = layernorm_ref(x, w, bias, eps, LN_BF16_DEPTH, sum_exact=True)
        got = ops.layernorm(x.to(dev), w.to(dev), None if bias is None else bias.to(dev), eps).cpu()
        ratio_check(f"layernorm offset rows dim={dim}", got, r["y"], layernorm_bf16_bound(r))
        const = (b if bias is not None else torch.zeros(dim)).bfloat16()
        assert bool((got[2].float() == const.float()).all()), "constant row"


# --------------------------------------------------------------------------------------------------------------------------- RoPE
def _rope_reference(qkv, cos, sin, S, H, D, pos0):
    """float64 [T, 3HD] reference and bound (zero on the v third: it has to keep its bits)."""
    T = qkv.shape[0]
    half = D // 2
    x = qkv.double()[:, :2 * H * D].view(T, 2 * H, 2, half)
    pos = torch.arange(T) % S + pos0
    c, s = cos.double()[pos][:, None, :], sin.double()[pos][:, None, :]
    rl, rh, bl, bh = rope_ref(x[:, :, 0], x[:, :, 1], c, s)
    ref = torch.cat([torch.stack([rl, rh], 2).reshape(T, 2 * H * D), qkv.double()[:, 2 * H * D:]], 1)
    bound = torch.cat([torch.stack([bl, bh], 2).reshape(T, 2 * H * D), torch.zeros(T, H * D, dtype=torch.float64)], 1)
    return ref, bound


@pytest.mark.parametrize("D", [16, 64, 128])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("pos0", [0, 5])
def test_rope_qk(dev, D, H, pos0):
    """Three sequences of S = 37 tokens (tok % S matters, the last block is partial), tables of random angles (every (position, column)
    pair distinct), ld = 3HD + 8 with canary columns; the v third keeps its bits."""
    from medplib_amd import ops
    S, T = 37, 3 * 37
    g = gen(D * 10 + H + pos0)
    qkv = torch.randn(T, 3 * H * D, generator=g).bfloat16()
    ang = torch.rand(S + pos0, D // 2, generator=g) * 6.283
    cos, sin = torch.cos(ang), torch.sin(ang)
    ref, bound = _rope_reference(qkv, cos, sin, S, H, D, pos0)
    ld = 3 * H * D + 8
    whole, view = canary_view(T, 3 * H * D, ld, torch.bfloat16, dev)
    view.copy_(qkv.to(dev))
    ops.rope_qk_(view, cos.to(dev), sin.to(dev), S, H, D, pos0)
    torch.cuda.synchronize()
    ratio_check(f"rope D={D} H={H} pos0={pos0}", view, ref, bound)
    assert_bits("rope: the v third", view[:, 2 * H * D:], qkv[:, 2 * H * D:])
    canary_intact("rope qkv", whole, T, 3 * H * D, ld)


def test_rope_short_table_raises(dev):
    from medplib_amd import ops
    from medplib_amd._lib import MedplibError
    S, H, D, pos0 = 37, 3, 64, 5
    qkv = torch.randn(2 * S, 3 * H * D, generator=gen(1)).bfloat16()
    buf = qkv.to(dev)
    tab = torch.rand(S + pos0 - 1, D // 2, generator=gen(2)).to(dev)
    with pytest.raises(MedplibError, match="table_rows"):
        ops.rope_qk_(buf, tab, tab, S, H, D, pos0)
    torch.cuda.synchronize()
    assert_bits("qkv after the refused call", buf, qkv)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("B", [1, 3])
def test_decode_rope_append_values(dev, D, B):
    """Value parity at position 0 and at the last cache row, into a cache whose sequence stride exceeds H * D; every other cache row
    and the gap columns keep their bits.  (Bounds on the position and the error word: test_gpu_long_context.py.)"""
    from medplib_amd import ops
    H, L, half = 3, 6, D // 2
    g = gen(D + B)
    ang = torch.rand(L, half, generator=g) * 6.283
    cos, sin = torch.cos(ang), torch.sin(ang)
    for pos in (0, L - 1):
        qkv = torch.randn(B, 3 * H * D, generator=g).bfloat16()
        wide_k = torch.full((B, L, H + 1, D), CANARY, dtype=torch.bfloat16, device=dev)
        wide_v = torch.full((B, L, H + 1, D), CANARY, dtype=torch.bfloat16, device=dev)
        ck, cv = wide_k[:, :, :H], wide_v[:, :, :H]                    # sequence stride (H + 1) D
        buf = qkv.to(dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        ops.decode_rope_append(buf, cos.to(dev), sin.to(dev), ck, cv, torch.tensor([pos], dtype=torch.int32, device=dev), H, D, err=err)
        torch.cuda.synchronize()
        assert int(err) == 0
        x = qkv.double()[:, :2 * H * D].view(B, 2 * H, 2, half)
        rl, rh, bl, bh = rope_ref(x[:, :, 0], x[:, :, 1], cos.double()[pos], sin.double()[pos])
        ref = torch.stack([rl, rh], 2).reshape(B, 2, H * D)
        bound = torch.stack([bl, bh], 2).reshape(B, 2, H * D)
        got = buf.cpu()
        ratio_check(f"decode rope q D={D} B={B} pos={pos}", got[:, :H * D], ref[:, 0], bound[:, 0])
        ratio_check(f"decode rope k D={D} B={B} pos={pos}", wide_k[:, pos, :H].reshape(B, H * D), ref[:, 1], bound[:, 1])
        assert_bits("decode: v in qkv", got[:, 2 * H * D:], qkv[:, 2 * H * D:])
        assert_bits("decode: v appended", wide_v[:, pos, :H].reshape(B, H * D), qkv[:, 2 * H * D:])
        for wide in (wide_k, wide_v):
            rest = wide.cpu().clone()
            rest[:, pos, :H] = CANARY
            assert_bits("decode: other cache rows and gap columns", rest, torch.full_like(rest, CANARY))


# ------------------------------------------------------------------------------------------------------------------------- SwiGLU
def _swiglu_check(name, got, gu, F):
    ref, ulp, floor = swiglu_ref(gu[:, :F].float(), gu[:, F:2 * F].float())
    err = (got.detach().cpu().double() - ref).abs()
    ulps = float(((err - floor).clamp_min(0) / ulp).max())
    i = int(((err - floor).clamp_min(0) / ulp).flatten().argmax())
    print(f"{name}: worst (err - floor) / bf16 ulp = {ulps:.3f} at g={float(gu[:, :F].flatten()[i]):.6g} u={float(gu[:, F:2 * F].flatten()[i]):.6g}, "
          f"worst err / ulp without the floor = {float((err / ulp).max()):.3f}")
    return ratio_check(name, got, ref, ulp + floor)


@pytest.mark.parametrize("F", [8, 264, 11008])
@pytest.mark.parametrize("rows", [1, 33])
def test_swiglu(dev, F, rows):
    from medplib_amd import ops
    gu = (2.5 * torch.randn(rows, 2 * F, generator=gen(F + rows))).bfloat16()
    got = ops.swiglu(gu.to(dev))
    whole, out = canary_view(rows, F, F + 16, torch.bfloat16, dev)
    got_s = ops.swiglu(strided_in(gu, 2 * F + 8, dev), out=out)
    torch.cuda.synchronize()
    _swiglu_check(f"swiglu F={F} rows={rows}", got, gu, F)
    assert_bits("swiglu strided == contiguous", got_s, got)
    canary_intact("swiglu out", whole, rows, F, F + 16)


def test_swiglu_sigmoid_sweep(dev):
    """Every finite bf16 g in [-100, 100] against u = 1, -1.5 and 3e4: one bf16 ulp of the exact value plus the flush-to-zero floor
    (kernel_parity.swiglu_ref).  MEASURED on MI355X: see profiles/row_kernel_parity_tests.md."""
    from medplib_amd import ops
    gu, n = swiglu_sweep()
    F = gu.shape[1] // 2
    got = ops.swiglu(gu.to(dev))
    torch.cuda.synchronize()
    assert n > 34000
    _swiglu_check("swiglu sweep", got, gu, F)


# -------------------------------------------------------------------------------------------------------------------------- casts
def test_cast_to_bf16_ties(dev):
    """Round to nearest even, bit for bit with torch on the CPU, around every tie: at the full length and with 1..3 elements cut (the
    scalar tail then holds ties), and at n = 1, 2, 3, 5."""
    from medplib_amd import ops
    sweep = cast_tie_sweep()
    ref = sweep.bfloat16()
    N = sweep.numel()
    for n in (N, N - 1, N - 2, N - 3):
        assert_bits_nan(f"cast_to_bf16 n={n} (n % 4 = {n % 4})", ops.cast_to_bf16(sweep[:n].clone().to(dev)), ref[:n])
    ties = sweep[-8:]
    for n in (1, 2, 3, 5):
        for start in (0, 1):                                              # a tie that rounds down first, then one that rounds up
            assert_bits_nan(f"cast_to_bf16 ties n={n} start={start}", ops.cast_to_bf16(ties[start:start + n].clone().to(dev)),
                            ref[N - 8 + start:N - 8 + start + n])


def test_cast_to_f32_all_patterns(dev):
    from medplib_amd import ops
    pat = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    got = ops.cast_to_f32(pat.to(dev))
    ref = (pat.view(torch.int16).to(torch.int32) << 16).view(torch.float32)          # exact by construction: the pattern in the high half
    assert_bits("cast_to_f32 all 65536 patterns", got, ref)


# ------------------------------------------------------------------------------------------------------------------ add_rows, add3
def _spaced_pairs(shape, seed):
    """(a, b) bf16 with |a| / |b| = 2^9 on every third element: the exact sum needs more than 8 bits and the fp32 sum is then rounded."""
    g = gen(seed)
    a = torch.randn(shape, generator=g).bfloat16()
    b = torch.randn(shape, generator=g).bfloat16()
    a.view(-1)[::3] = (b.view(-1)[::3].float() * 512).bfloat16()
    return a, b


@pytest.mark.parametrize("dim", [8, 24, 1024])
@pytest.mark.parametrize("period", [1, 3, 0])
def test_add_rows(dev, dim, period):
    from medplib_amd import ops
    rows = 9
    period = period or rows
    x, _ = _spaced_pairs((rows, dim), dim + period)
    add = (x[:period].float() / 512 * (1 + torch.arange(period).float()[:, None])).bfloat16()
    got = ops.add_rows(x.to(dev), add.to(dev))
    ref = (x.float() + add.float().repeat(rows // period, 1)).bfloat16()
    assert_bits(f"add_rows dim={dim} period={period}", got, ref)
    assert int((ref.float() != x.float()).sum()) > 0


@pytest.mark.parametrize("n", [8, 2048, 2056])
@pytest.mark.parametrize("with_c", [True, False])
def test_add3(dev, n, with_c):
    from medplib_amd import ops
    a, b = _spaced_pairs((n,), n)
    c = torch.randn(n, generator=gen(n + 1)).bfloat16()
    whole = torch.full((n + 16,), CANARY, dtype=torch.bfloat16, device=dev)
    out = whole[8:8 + n]
    got = ops.add3(a.to(dev), b.to(dev), c.to(dev) if with_c else None, out=out)
    ref = (a.float() + b.float()) + (c.float() if with_c else 0.0)
    assert_bits(f"add3 n={n} c={with_c}", got, ref.bfloat16())
    canary_intact("add3 out", whole, 1, n, n + 8)


@pytest.mark.parametrize("n", [1, 64])
def test_advance_ints(dev, n):
    from medplib_amd import ops
    v = torch.randint(-1000, 1000, (n + 2,), generator=gen(n), dtype=torch.int32)
    buf = v.to(dev)
    ops.advance_ints(buf[1:1 + n], -7)
    ops.advance_ints(buf[1:1 + n], 3)
    ref = v.clone()
    ref[1:1 + n] += -4
    assert_bits(f"advance_ints n={n}", buf, ref)
