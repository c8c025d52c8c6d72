"""Kernel-level parity of the trunk's index-driven glue kernels (glue_ops.hip, norm_elementwise.hip, the upsampler's weight pack):
equal bits with torch indexing / arithmetic at the documented rounding points; the kernels that add or average round fp32 math to bf16
once.  Wherever a kernel writes a sub-range of a buffer, sentinel bands in front of and behind it must come back unchanged.
Valid indices only: none of these kernels bound-checks."""
import math

import pytest
import torch
import torch.nn.functional as F

from kernel_parity import BF16_RTOL, U32, assert_bits, bf, report

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _banded(dev, shape, fill=-9.0, dtype=torch.bfloat16):
    """(whole buffer, the inner view a kernel may write): one sentinel row block before and after."""
    rows = shape[0]
    whole = torch.full((rows + 2,) + tuple(shape[1:]), fill, dtype=dtype, device=dev)
    return whole, whole[1:rows + 1]


def _bands_intact(whole, fill=-9.0):
    w = whole.cpu().float()
    assert bool((w[0] == fill).all() and (w[-1] == fill).all()), "a sentinel band next to the output was written"


def test_splice_rows(dev):
    from medplib_amd import _lib, ops
    g = _gen(1)
    dim, vocab, nf = 72, 40, 13
    embed = torch.randn(vocab, dim, generator=g).bfloat16(); feats = torch.randn(nf, dim, generator=g).bfloat16()
    PAD = ops.SPLICE_PAD
    for first, last in ((0, -1 - (nf - 1)), (-1 - 0, PAD), (PAD, vocab - 1)):      # each kind of code in the first and in the last row
        mid = [vocab - 1, 0, -1, -nf, PAD, 5, -3, PAD, 17]
        code = torch.tensor([first] + mid + [last], dtype=torch.int64)
        whole, out = _banded(dev, (code.numel(), dim))
        e_d, f_d, c_d = embed.to(dev), feats.to(dev), code.to(dev)          # held: a temporary would be freed before the kernel runs
        _lib.lib().call("mp_splice_rows_bf16", e_d.data_ptr(), f_d.data_ptr(), c_d.data_ptr(), out.data_ptr(), code.numel(), dim, ops._stream())
        got = ops.splice_rows(e_d, f_d, c_d, dim)
        torch.cuda.synchronize()
        ref = torch.zeros(code.numel(), dim, dtype=torch.bfloat16)
        for r, c in enumerate(code.tolist()):
            if c == PAD:
                continue
            ref[r] = embed[c] if c >= 0 else feats[-1 - c]
        assert {"e" if c >= 0 else ("p" if c == PAD else "f") for c in code.tolist()} == {"e", "f", "p"}
        assert_bits("splice_rows", got, ref)
        assert_bits("splice_rows (banded)", out, ref)
        _bands_intact(whole)


@pytest.mark.parametrize("patch,grid", [(14, 3), (16, 2)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_patch_im2col(dev, patch, grid, dtype):
    """CLIP (14 x 14) and SAM (16 x 16) patch geometry: bf16 of the pixel in Conv2d's weight.view(out, -1) column order, zero padding columns."""
    from medplib_amd import ops
    g = _gen(patch)
    B, C = 2, 3
    H, W = grid * patch, (grid + 1) * patch
    k = C * patch * patch
    kp = (k + 63) // 64 * 64 + 64
    assert kp > k
    img = torch.randn(B, C, H, W, generator=g).to(dtype)
    cols = ops.patch_im2col(img.to(dev), patch, kp)
    torch.cuda.synchronize()
    ref = torch.zeros(B * grid * (grid + 1), kp, dtype=torch.bfloat16)
    ref[:, :k] = F.unfold(img.float(), patch, stride=patch).transpose(1, 2).reshape(-1, k).bfloat16()      # unfold: (c, py, px) order
    assert_bits(f"patch_im2col p={patch} {dtype}", cols, ref)
    assert bool((cols.cpu()[:, k:] == 0).all())
    # the column order IS the convolution's: a patch-embedding conv equals cols @ weight.view(out, -1)^T
    wt = torch.randn(5, C, patch, patch, generator=g).double()
    conv = F.conv2d(img.bfloat16().double(), wt, stride=patch).permute(0, 2, 3, 1).reshape(-1, 5)
    viaf = cols.cpu().double()[:, :k] @ wt.view(5, -1).t()
    assert torch.allclose(conv, viaf, rtol=1e-12, atol=1e-12)


def test_window_unpartition_add(dev):
    """The 16-token grid with 14-token windows (H, W not multiples of ws): out = bf16(win[window cell] + shortcut); the round trip through
    window_partition returns x + shortcut, and the padded cells are never read back."""
    from medplib_amd import _lib, ops
    g = _gen(3)
    for B, H, W, C, ws in ((2, 16, 16, 24, 14), (1, 15, 17, 8, 14), (1, 14, 28, 8, 14)):
        x = torch.randn(B, H, W, C, generator=g).bfloat16(); sc = torch.randn(B, H, W, C, generator=g).bfloat16()
        win = ops.window_partition(x.to(dev), ws)
        nwy, nwx = -(-H // ws), -(-W // ws)
        # partition: torch reference (zero padded)
        xp = torch.zeros(B, nwy * ws, nwx * ws, C, dtype=torch.bfloat16)
        xp[:, :H, :W] = x
        wref = xp.view(B, nwy, ws, nwx, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B * nwy * nwx, ws * ws, C)
        assert_bits("window_partition", win, wref)
        win2 = torch.randn(wref.shape, generator=g).bfloat16()            # independent window contents, padding cells non-zero on purpose
        whole, out = _banded(dev, (B * H, W, C))
        w2_d, sc_d = win2.to(dev), sc.to(dev)
        _lib.lib().call("mp_window_unpartition_add_bf16", w2_d.data_ptr(), sc_d.data_ptr(), out.data_ptr(), B, H, W, C, ws, ops._stream())
        rt = ops.window_unpartition_add(win, sc_d, ws)
        torch.cuda.synchronize()
        un = win2.view(B, nwy, nwx, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, nwy * ws, nwx * ws, C)[:, :H, :W]
        assert_bits(f"window_unpartition_add {H}x{W}", out.view(B, H, W, C), bf(un.float() + sc.float()).bfloat16())
        _bands_intact(whole)
        assert_bits("window round trip", rt, bf(x.float() + sc.float()).bfloat16())


def test_clip_embed_and_copy_rows(dev):
    from medplib_amd import ops
    g = _gen(4)
    B, NP, C = 3, 16, 40
    patch = torch.randn(B, NP, C, generator=g).bfloat16(); cls = torch.randn(C, generator=g).bfloat16()
    pos = torch.randn(NP + 1, C, generator=g).bfloat16()
    emb = ops.clip_embed(patch.to(dev), cls.to(dev), pos.to(dev), B, NP, C)
    ref = torch.cat([cls.float().expand(B, 1, C), patch.float()], dim=1) + pos.float()[None]
    assert_bits("clip_embed", emb, bf(ref).bfloat16())
    # drop the CLS row of every image (B > 1)
    rows = ops.copy_rows(emb.view(-1, C), B * NP, C, NP, NP + 1, 1)
    torch.cuda.synchronize()
    assert_bits("copy_rows (CLS dropped)", rows, emb.cpu()[:, 1:].reshape(B * NP, C))
    # a general window: rows 2..5 of every batch of 7
    src = torch.randn(4 * 7, C, generator=g).bfloat16()
    got = ops.copy_rows(src.to(dev), 4 * 4, C, 4, 7, 2)
    torch.cuda.synchronize()
    assert_bits("copy_rows window", got, src.view(4, 7, C)[:, 2:6].reshape(16, C))


@pytest.mark.parametrize("Lin,Lout", [(576, 256), (441, 64), (64, 64)])
def test_adaptive_avgpool_tokens(dev, Lin, Lout):
    """nn.AdaptiveAvgPool1d over the token axis in float64: an fp32 chain of window-size additions (<= ceil(Lin / Lout) + 1), a product with the
    rounded reciprocal, one bf16 rounding."""
    from medplib_amd import ops
    g = _gen(Lin + Lout)
    n, C = 2, 72
    x = torch.randn(n, Lin, C, generator=g).bfloat16()
    got = ops.adaptive_avgpool_tokens(x.to(dev), Lout)
    torch.cuda.synchronize()
    pool = torch.nn.AdaptiveAvgPool1d(Lout)
    ref = pool(x.double().permute(0, 2, 1)).permute(0, 2, 1)
    mag = pool(x.double().abs().permute(0, 2, 1)).permute(0, 2, 1)
    win = -(-Lin // Lout) + 1
    report(f"adaptive_avgpool_tokens {Lin}->{Lout}", got, ref, rtol=BF16_RTOL, atol=(win + 2) * U32 * mag)


@pytest.mark.parametrize("img_dtype", [torch.bfloat16, torch.float32])
def test_conv3x3s2_c1_gelu(dev, img_dtype):
    """The inference-side first layer of the MaskTokenEncoder equals the training forward's two kernels, gelu_fwd_bf16(conv3x3s2_c1_pre), to
    the bf16 bit (the bf16 module rounds the convolution's output before the GELU), and the float64 conv + erf-GELU within: one bf16 rounding
    of the pre-activation carried through the GELU (slope <= 1.13) + the GELU fit's documented absolute error + one output rounding."""
    from medplib_amd import ops
    from medplib_amd.model import icl
    from medplib_amd.model.config import MedPLIBConfig
    S, CO = MedPLIBConfig().clip_image_size, icl.MaskTokenEncoder.CH[0]
    for n, H, W, co in ((2, 7, 9, 16), (1, 8, 10, 8), (1, S, S, CO)):
        g = _gen(H + W)
        img = (torch.rand(n, H, W, generator=g) * 2 - 0.5).to(img_dtype)
        wt = torch.randn(co, 9, generator=g) / 3; b = torch.randn(co, generator=g) * 0.1
        fused = ops.conv3x3s2_c1_gelu(img.to(dev), wt.to(dev), b.to(dev))
        two = ops.gelu_fwd_bf16(ops.conv3x3s2_c1_pre(img.to(dev), wt.to(dev), b.to(dev)))
        torch.cuda.synchronize()
        assert_bits(f"conv3x3s2_c1_gelu == gelu(pre) {img_dtype} {H}x{W}", fused, two)
        x64 = img.bfloat16().double()[:, None]
        pre = F.conv2d(x64, wt.double().view(co, 1, 3, 3), b.double(), stride=2, padding=1).permute(0, 2, 3, 1)
        mag = F.conv2d(x64.abs(), wt.double().abs().view(co, 1, 3, 3), b.double().abs(), stride=2, padding=1).permute(0, 2, 3, 1)
        ref = 0.5 * pre * torch.special.erfc(-pre / math.sqrt(2.0))
        atol = 1.13 * (2.0 ** -9 * pre.abs() + 10 * U32 * mag) + 4.8e-7
        report(f"conv3x3s2_c1_gelu vs float64 {img_dtype} {H}x{W}", fused, ref, rtol=BF16_RTOL, atol=atol)


def test_cast_and_scale(dev):
    from medplib_amd import ops
    g = _gen(6)
    for n in (1, 7, 8, 1031):
        x = (torch.randn(n, generator=g) * 100).bfloat16()
        assert_bits(f"cast_to_f32 n={n}", ops.cast_to_f32(x.to(dev)), x.float())
        y = torch.randn(n, generator=g)
        whole, inner = _banded(dev, (n,), fill=-9.0, dtype=torch.float32)
        inner.copy_(y.to(dev))
        ops.scale_f32_(inner, 0.3)
        torch.cuda.synchronize()
        assert_bits(f"scale_f32_ n={n}", inner, y * torch.tensor(0.3, dtype=torch.float32))
        _bands_intact(whole)


def test_pack_upsampler_weights_all(dev):
    """[Cin, Cout, 2, 2] fp32 -> [(kh, kw, cout), cin] bf16 = permute(2, 3, 1, 0), and its transpose, for both layers in one launch."""
    from medplib_amd import ops
    g = _gen(7)
    w1 = torch.randn(256, 64, 2, 2, generator=g); w2 = torch.randn(64, 32, 2, 2, generator=g)
    w1p, w2p, w1t, w2t = ops.pack_upsampler_weights_all(w1.to(dev), w2.to(dev))
    torch.cuda.synchronize()
    for name, w, wp, wt in (("w1", w1, w1p, w1t), ("w2", w2, w2p, w2t)):
        ref = w.permute(2, 3, 1, 0).reshape(4 * w.shape[1], w.shape[0]).contiguous().bfloat16()
        assert_bits(f"upsampler pack {name}", wp, ref)
        assert_bits(f"upsampler pack {name}^T", wt, ref.t().contiguous())
    a, b = ops.pack_upsampler_weights(w1.to(dev), w2.to(dev))
    assert_bits("pack_upsampler_weights (torch form) agrees", a, w1p.cpu())


def test_gate_noise_dev_equals_host_keyed(dev):
    """The device-keyed draws (offset = pass_dev[0] * stride) are the host-keyed launch's, bit for bit, uniform and Gumbel.
    mp_gate_noise_dev_f32 had no test that called it (the coverage guard named it); this pins it to the host-keyed kernel, which is an
    equivalence, not an independent reference: the draws themselves are a hash whose distribution test_gpu_decode_top2 exercises."""
    from medplib_amd import ops
    for gumbel in (False, True):
        for n, seed, p, stride in ((1, 3, 0, 64), (257, 11, 5, 40), (4096, 12345, 77, 4096)):
            pd = torch.tensor([p], dtype=torch.int32, device=dev)
            a = ops.gate_noise_dev(n, seed, pd, stride, gumbel, dev)
            b = ops.gate_noise(n, seed, p * stride, gumbel, dev)
            torch.cuda.synchronize()
            assert_bits(f"gate_noise_dev n={n} gumbel={gumbel}", a, b)
            assert bool(torch.isfinite(a).all())


def test_rope_qk_unbounded_equals_bounded(dev):
    """mp_rope_qk_bf16 (no table-length argument) is kept in the C ABI beside the bounded form every Python caller uses (ops.rope_qk_, whose
    parity with the oracle test_gpu_trunk_kernels pins): the same bits on a table that is long enough, and nothing outside the q and k thirds
    of the fused rows is touched."""
    from medplib_amd import _lib, ops
    g = _gen(9)
    B, S, H, D, pos0 = 2, 37, 3, 64, 5
    qkv = torch.randn(B * S, 3 * H * D, generator=g).bfloat16()
    ang = torch.rand(S + pos0 + 3, D // 2, generator=g) * 6.0
    cos_t, sin_t = ang.cos().to(dev), ang.sin().to(dev)
    a = qkv.to(dev).clone(); b = qkv.to(dev).clone()
    ops.rope_qk_(a, cos_t, sin_t, S, H, D, pos_offset=pos0)
    _lib.lib().call("mp_rope_qk_bf16", b.data_ptr(), b.stride(0), cos_t.data_ptr(), sin_t.data_ptr(), b.shape[0], S, H, D, pos0, ops._stream())
    torch.cuda.synchronize()
    assert_bits("rope_qk: unbounded == bounded", b, a)
    assert_bits("rope_qk leaves v alone", b[:, 2 * H * D:], qkv[:, 2 * H * D:])
    assert not torch.equal(b.cpu()[:, :2 * H * D], qkv[:, :2 * H * D])
