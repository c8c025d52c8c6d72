"""The decode GEMV family at every launch edge: mp_gemv_bf16 and mp_gemv_w8_bf16 in their shared, indexed and K-split forms,
mp_gemv_top2_gate_up_bf16 / mp_gemv_top2_down_bf16 and mp_quantize_rows_w8_bf16, on the cases of tests/gemv_cases.py (ragged N down to one
row, five to eight x rows, every edge of the K loops, both sides of the K-split predicate, every capacity-drop pattern).

No tolerance, except where SwiGLU's fast sigmoid stands between the operands and the result: on grid operands every dot product is one exact
fp32 number whatever the summation order, so a kernel must EQUAL the float64 reference of its epilogue, and two kernels that compute the
same product must return the same bits.

Guard bands.  The entry points are called directly with every operand a view into a larger arena: x, W, codes and the residual have padded
leading dimensions and a guard row, filled with NaN (codes: 127 under a NaN scale); the matrices of experts no row selects are NaN; w_index,
row_scale, row_keep and the bias sit between poison entries; the output is the corner of an arena prefilled with a NaN bit pattern no kernel
produces.  A read from any guard turns an output NaN or wrong, a store outside [0, M) x [0, N) changes a sentinel.  All of it is ordinary
allocated memory and every call satisfies the entry points' own preconditions."""
import math
from types import SimpleNamespace

import pytest
import torch

import gemv_cases as C
from oracle import ops as O
from test_gpu_w8_gemv import _quant_ref

pytestmark = pytest.mark.gpu

BF16_EPS = 2.0 ** -8
MP_BF16, MP_F32 = 0, 1
S16, S32, S8 = 0x7FC1, 0x7FC00001, 0x5A                       # sentinels: two NaN patterns no arithmetic here produces, and a byte
NAN = float("nan")


def _call(name, *args):
    from medplib_amd._lib import lib
    lib().call(name, *args, torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _padded(data, pad, fill):
    """data [R, C] in the corner of [R + 1, C + pad] of `fill`."""
    R, Cc = data.shape
    a = torch.full((R + 1, Cc + pad), fill, dtype=data.dtype)
    a[:R, :Cc] = data
    return a


def _mid(values, poison, dtype, dev):
    """`values` between five poison entries on either side -> (the device array, the address of values[0])."""
    v = torch.as_tensor(values).to(dtype)
    a = torch.full((v.numel() + 10,), poison, dtype=dtype)
    a[5:5 + v.numel()] = v
    d = a.to(dev)
    return d, d[5:].data_ptr()


def _weights(o, w8, dev):
    """The weight arena of o on the device, built once: [E][N + 1, K + 16] with the stride between experts a multiple of 16 elements; bf16:
    NaN outside [N, K] and in every expert no row selects; int8: code 127 there, and scale [E, N + 1] NaN there.  The scales are 2^e of the
    grid, or o.scale where the rows are no grid rows."""
    cache = o.__dict__.setdefault("_dev", {})
    if w8 not in cache:
        w = o.c.to(torch.int8) if w8 else o.w
        rs = o.scale if getattr(o, "scale", None) is not None else C.pow2(o.e)
        if w.dim() == 2:
            w, rs, selected = w.unsqueeze(0), rs.unsqueeze(0), [0]
        else:
            selected = sorted(set(o.idx if getattr(o, "idx", None) is not None else o.expert))
        E_, N, K = w.shape
        ldw = K + 16
        stride = ((N + 1) * ldw + 15) // 16 * 16
        a = torch.full((E_ * stride,), 127 if w8 else NAN, dtype=w.dtype)
        for s in selected:
            a[s * stride:s * stride + (N + 1) * ldw].view(N + 1, ldw)[:N, :K] = w[s]
        sc = None
        if w8:
            sc = torch.full((E_, N + 1), NAN)
            for s in selected:
                sc[s, :N] = rs[s]
            sc = sc.to(dev)
        cache[w8] = (a.to(dev), ldw, stride if E_ > 1 else 0, sc, N + 1 if E_ > 1 else 0)
    return cache[w8]


def _out_arena(rows, cols, f32, dev):
    return torch.full((rows + 1, cols + 8), S32 if f32 else S16, dtype=torch.int32 if f32 else torch.int16, device=dev)


def _take(y, rows, cols, f32, tag, unwritten=()):
    """The [rows, cols] corner of an output arena after the launch.  Everything else still holds the sentinel, so do the `unwritten` rows;
    no other row holds a NaN."""
    torch.cuda.synchronize()
    a = y.cpu()
    s = S32 if f32 else S16
    outside = torch.ones_like(a, dtype=torch.bool)
    outside[:rows, :cols] = False
    assert bool((a[outside] == s).all()), (tag, "a store outside [0, M) x [0, N)")
    inside = a[:rows, :cols].contiguous()
    for m in unwritten:
        assert bool((inside[m] == s).all()), (tag, m, "a dropped row was written")
    vals = inside.view(torch.float32 if f32 else torch.bfloat16)
    checked = [m for m in range(rows) if m not in unwritten]
    assert not bool(torch.isnan(vals[checked]).any()), (tag, "NaN: a guard was read or an element was not written")
    return vals


def _gemv(dev, o, w8, act=C.ACT_NONE, f32=False, alpha=1.0, bias=False, res=False, scale=False, keep=None, x=None, idx=None,
          unwritten=()):
    """One launch of mp_gemv_bf16 / mp_gemv_w8_bf16 on o's operands inside their guard bands -> y [M, N or N / 2] on the CPU."""
    x = o.x if x is None else x
    idx = getattr(o, "idx", None) if idx is None else idx
    M, K, N = x.shape[0], o.K, o.N
    n_out = N // 2 if act == C.ACT_SWIGLU_PAIR else N
    tag = (o.N, o.K, M, "int8" if w8 else "bf16", act, f32, alpha, bias, res, scale, keep, idx)
    W, ldw, strideW, sc, strideScale = _weights(o, w8, dev)
    xd = _padded(x, 8, NAN).to(dev)
    rd = _padded(o.res[:M], 8, NAN).to(dev) if res else None
    y = _out_arena(M, n_out, f32, dev)
    hold = [_mid(o.bias, NAN, torch.float32, dev) if bias else (None, None),
            _mid(idx, C.E + 7, torch.int32, dev) if idx is not None else (None, None),
            _mid(o.row_scale[:M], NAN, torch.float32, dev) if scale else (None, None),
            _mid(keep, -1, torch.int32, dev) if keep is not None else (None, None)]
    (_, bias_p), (_, idx_p), (_, scale_p), (_, keep_p) = hold
    tail = (y.data_ptr(), y.stride(0), bias_p, rd.data_ptr() if res else None, rd.stride(0) if res else 0, idx_p, scale_p, keep_p, M, N, K, act,
            MP_F32 if f32 else MP_BF16, float(alpha))
    if w8:
        _call("mp_gemv_w8_bf16", xd.data_ptr(), xd.stride(0), W.data_ptr(), ldw, strideW, sc.data_ptr(), strideScale, *tail)
    else:
        _call("mp_gemv_bf16", xd.data_ptr(), xd.stride(0), W.data_ptr(), ldw, strideW, *tail)
    return _take(y, M, n_out, f32, tag, unwritten)


def _dropped(keep):
    return [m for m, s in enumerate(keep) if s < 0]


def _within(name, got, ref, rtol, atol):
    got, ref = got.float(), ref.float()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    msg = f"{name}: max|err|={err.max().item():.4e}, ref absmax={ref.abs().max().item():.4e}, bad={int(bad.sum())}/{bad.numel()}"
    assert not bad.any(), msg


# ------------------------------------------------------------------------------------------------ 1. shared forms
def _shared_variants(w8):
    v = [dict(), dict(f32=True), dict(res=True), dict(f32=True, res=True), dict(alpha=0.5), dict(alpha=0.5, f32=True, res=True)]
    if not w8:                                                  # (the int8 entry refuses a bias and ReLU)
        v += [dict(bias=True), dict(bias=True, act=C.ACT_RELU), dict(bias=True, act=C.ACT_RELU, alpha=0.5, res=True),
              dict(bias=True, alpha=0.5, f32=True), dict(bias=True, act=C.ACT_RELU, f32=True, res=True)]
    return v


@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "int8"])
def test_shared_forms_equal_the_float64_reference(dev, w8):
    """One matrix for one to eight rows (five to eight: two passes, the second on offset x, y and residual), and the K-split kernel at one
    row with a long K: bf16 and fp32 output, residual, alpha = 0.5, and for bf16 weights a bias under NONE and ReLU."""
    for case in C.shared_cases(w8):
        o = C.operands(case)
        for kw in _shared_variants(w8):
            got = _gemv(dev, o, w8, **kw)
            ref = C.ref_shared(o.a, kw.get("alpha", 1.0), o.bias if kw.get("bias") else None, kw.get("act", C.ACT_NONE),
                               o.res if kw.get("res") else None, kw.get("f32", False))
            assert torch.equal(got, ref), (case, kw)


# ------------------------------------------------------------------------------------------------ 2. indexed forms
@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "int8"])
def test_indexed_forms_equal_the_float64_reference(dev, w8):
    """A matrix per row (the wave-per-four-rows kernel and the K-split kernel) under every keep pattern, with and without a residual: the
    combine weight on the bf16-rounded product, then the residual.  A dropped row is the residual's bits, +0 without one."""
    for case in C.indexed_cases(w8):
        o = C.operands(case)
        got = _gemv(dev, o, w8)                                 # no row_scale, no row_keep, no residual: the null paths
        assert torch.equal(got, C.ref_indexed(o.a)), case
        for name, keep in C.keep_patterns(case.M).items():
            for res in (True, False):
                got = _gemv(dev, o, w8, res=res, scale=True, keep=keep)
                ref = C.ref_indexed(o.a, o.row_scale, o.res if res else None, keep)
                assert torch.equal(got, ref), (case, name, res)
                for m in _dropped(keep):
                    want = o.res[m] if res else torch.zeros(case.N, dtype=torch.bfloat16)
                    assert torch.equal(_bits(got[m]), _bits(want)), (case, name, res, m, "a dropped row is the residual's bits, or +0")


# ------------------------------------------------------------------------------------------------ 3. one product, one result
def test_every_route_returns_the_same_bits(dev):
    """Across each term of `N <= 4096 && K >= 4096 && (w_index || M == 1)`: the K-split kernel and the wave-per-four-rows kernel on the same
    sums return the same bits (and the reference's).  Over the whole table (every case whose K both entries accept): mp_gemv_w8_bf16 on the
    codes of the grid weights equals mp_gemv_bf16 on the weights, and a second launch of either equals the first."""
    for w8 in (False, True):
        for term, left, right, rows, cols in C.predicate_pairs(w8):
            assert C.route(left.M, left.N, left.K, False, False, w8)[0] == "ksplit" and C.route(right.M, right.N, right.K, False, False, w8)[0] == "shared"
            for kw in (dict(), dict(f32=True), dict(res=True)):
                a, b = _gemv(dev, left, w8, **kw), _gemv(dev, right, w8, **kw)
                assert torch.equal(_bits(a[:rows, :cols]), _bits(b[:rows, :cols])), (term, w8, kw)
                ref = C.ref_shared(left.a, residual=left.res if kw.get("res") else None, out_f32=kw.get("f32", False))
                assert torch.equal(a, ref), (term, w8, kw)
    for case in C.both_types_cases():
        o = C.operands(case)
        if case.indexed:
            pats = C.keep_patterns(case.M)
            variants = [dict(res=True, scale=True, keep=pats["none"]), dict(res=True, scale=True, keep=pats["first"]),
                        dict(scale=True, keep=[-1] * case.M)]
        else:
            variants = [dict(), dict(f32=True), dict(res=True)]
        for kw in variants:
            b, q = _gemv(dev, o, False, **kw), _gemv(dev, o, True, **kw)
            assert torch.equal(_bits(b), _bits(q)), (case, kw)
            assert torch.equal(_bits(_gemv(dev, o, False, **kw)), _bits(b)) and torch.equal(_bits(_gemv(dev, o, True, **kw)), _bits(q)), (case, kw)


# ------------------------------------------------------------------------------------------------ 4. SwiGLU forms
def _top2_gate_up(dev, o, slot):
    """mp_gemv_top2_gate_up_bf16 on o (x [T, K], 2T entries) -> act [2T, N / 2]; the rows of dropped entries must keep the sentinel."""
    W, ldw, strideW, _, _ = _weights(o, False, dev)
    xd = _padded(o.x, 8, NAN).to(dev)
    y = _out_arena(2 * o.T, o.N // 2, False, dev)
    (ed, ep), (sd, sp) = _mid(o.expert, C.E + 7, torch.int32, dev), _mid(slot, -1, torch.int32, dev)
    _call("mp_gemv_top2_gate_up_bf16", xd.data_ptr(), xd.stride(0), W.data_ptr(), ldw, strideW, y.data_ptr(), y.stride(0), ep, sp, o.T, o.N, o.K)
    return _take(y, 2 * o.T, o.N // 2, False, ("top2_gate_up", o.T, o.N, o.K, slot), unwritten=_dropped(slot))


def test_swiglu_forms_at_ragged_rows_and_drops(dev):
    """SwiGLU goes through mp_sigmoid_fast, so no float64 equality.  Shared form, M = 1..8: bf16 and int8 agree bit for bit on grid
    operands, and either is within the tolerance of test_gemv_decode_projections of the oracle — on grid operands (measured: the worst
    element at 0.95 of it, gate -6.4 against up -372, where the gate's bf16 rounding ahead of SiLU is what counts) and on random operands
    of that test's distribution, for which the tolerance was set (int8: the oracle sees code * scale).  Indexed form under
    every drop pattern: kept rows are the same bits in the int8 kernel, the bf16 kernel and mp_gemv_top2_gate_up_bf16; a dropped row stays
    unwritten in all three."""
    g = C.gen(900)
    for i, (M, N, K) in enumerate(C.SWIGLU_SHARED):
        o = C.operands(C.Case(False, False, M, N, K, 600 + i))
        b, q = _gemv(dev, o, False, act=C.ACT_SWIGLU_PAIR), _gemv(dev, o, True, act=C.ACT_SWIGLU_PAIR)
        assert b.shape == (M, N // 2) and torch.equal(_bits(b), _bits(q)), (M, N, K)
        gate, up = C.swiglu_halves(o.w.float())
        _within(f"swiglu shared grid {M}x{N}x{K}", b, O.swiglu(O.linear(o.x.float(), gate), O.linear(o.x.float(), up)), rtol=3 * BF16_EPS, atol=2e-2)
        # random operands (x ~ N(0, 1), products ~ N(0, 3.2) as in test_gemv_decode_projections); int8: the oracle sees code * scale
        x = torch.randn(M, K, generator=g).to(torch.bfloat16)
        w = (torch.randn(N, K, generator=g) * (3.2 / math.sqrt(K))).to(torch.bfloat16)
        codes, scale = _quant_ref(w)
        for w8, wf in ((False, w.float()), (True, codes.float() * scale.unsqueeze(-1))):
            r = SimpleNamespace(N=N, K=K, x=x, w=w, c=codes, scale=scale)
            gate, up = C.swiglu_halves(wf)
            ref = O.swiglu(O.linear(x.float(), gate), O.linear(x.float(), up))
            _within(f"swiglu shared {'int8' if w8 else 'bf16'} {M}x{N}x{K}", _gemv(dev, r, w8, act=C.ACT_SWIGLU_PAIR), ref, rtol=3 * BF16_EPS, atol=2e-2)
    for i, (T, N, K) in enumerate(C.SWIGLU_INDEXED):
        o = C.top2_operands(T, N, K, 800 + i, True)
        for name, slot in C.top2_patterns(T).items():
            act = _top2_gate_up(dev, o, slot)
            for c in range(2):
                sl, ex = slot[c * T:(c + 1) * T], o.expert[c * T:(c + 1) * T]
                q = _gemv(dev, o, True, act=C.ACT_SWIGLU_PAIR, idx=ex, keep=sl, unwritten=_dropped(sl))
                b = _gemv(dev, o, False, act=C.ACT_SWIGLU_PAIR, idx=ex, keep=sl, unwritten=_dropped(sl))
                kept = [t for t in range(T) if sl[t] >= 0]
                assert torch.equal(_bits(q[kept]), _bits(b[kept])), (T, N, K, name, c)
                assert torch.equal(_bits(q[kept]), _bits(act[c * T:(c + 1) * T][kept])), (T, N, K, name, c)


# ------------------------------------------------------------------------------------------------ 5. top-2 down + combine
def test_top2_down_at_ragged_rows_and_tails(dev):
    """mp_gemv_top2_down_bf16 (always the K-split layout) at N in {3, 17, 66}, K with equal parts, a lane-0 tail, unequal parts and below one
    step, T in {1, 3, 8}, under every drop pattern, with and without a residual: equal to the float64 reference; a token with both choices
    dropped is the residual's bits; the act rows of dropped entries are NaN and are never read."""
    for i, (T, N, K) in enumerate(C.TOP2_DOWN):
        o = C.top2_operands(T, N, K, 700 + i, False)
        dots = C.dot64_indexed(o.x, o.w, o.expert)
        W, ldw, strideW, _, _ = _weights(o, False, dev)
        for name, slot in C.top2_patterns(T).items():
            x = o.x.clone()
            for e in _dropped(slot):
                x[e] = NAN                                      # what mp_gemv_top2_gate_up_bf16 leaves unwritten
            xd = _padded(x, 8, NAN).to(dev)
            for res in (True, False):
                rd = _padded(o.res, 8, NAN).to(dev) if res else None
                y = _out_arena(T, N, False, dev)
                (ed, ep), (sd, sp), (wd, wp) = (_mid(o.expert, C.E + 7, torch.int32, dev), _mid(slot, -1, torch.int32, dev),
                                                _mid(o.weight, NAN, torch.float32, dev))
                _call("mp_gemv_top2_down_bf16", xd.data_ptr(), xd.stride(0), W.data_ptr(), ldw, strideW, y.data_ptr(), y.stride(0),
                      rd.data_ptr() if res else None, rd.stride(0) if res else 0, ep, sp, wp, T, N, K)
                got = _take(y, T, N, False, ("top2_down", T, N, K, name, res))
                assert torch.equal(got, C.ref_top2_down(dots, o.weight, slot, o.res if res else None)), (T, N, K, name, res)
                for t in range(T):
                    if res and slot[t] < 0 and slot[T + t] < 0:
                        assert torch.equal(_bits(got[t]), _bits(o.res[t])), (T, N, K, name, t)


# ------------------------------------------------------------------------------------------------ 6. the quantiser
def test_quantiser_strides_and_guards(dev):
    """mp_quantize_rows_w8_bf16 with ldw = K + 16 and ldc = K + 32 at K = 16 (one thread has work), 240 (the last thread idle), 256 (exactly
    one pass) and 272 (a second pass for sixteen threads), one and three rows: codes and scales equal the fp32 formula, on grid rows they
    are (c, 2^e), and no byte of the padding, of the guard rows or beside the scales changes."""
    g = C.gen(950)
    for rows in C.QUANT_ROWS:
        for K in C.QUANT_K:
            wr = (torch.randn(rows, K, generator=g) * 0.05).to(torch.bfloat16)
            wr[rows - 1, K // 2:] = 0
            if rows > 1:
                wr[1] = 0                                       # an all-zero row: scale 0, codes 0
            wg, c, e = C.grid(g, rows, K)
            for w, is_grid in ((wr, False), (wg, True)):
                src = _padded(w, 16, NAN).to(dev)
                codes = torch.full((rows + 1, K + 32), S8, dtype=torch.int8, device=dev)
                scale = torch.full((rows + 10,), S32, dtype=torch.int32, device=dev)
                _call("mp_quantize_rows_w8_bf16", src.data_ptr(), src.stride(0), rows, K, codes.data_ptr(), codes.stride(0), scale[5:].data_ptr())
                torch.cuda.synchronize()
                rc, rs = _quant_ref(w)
                cd, sd = codes.cpu(), scale.cpu()
                assert torch.equal(cd[:rows, :K], rc), (rows, K)
                assert torch.equal(sd[5:5 + rows].view(torch.float32), rs), (rows, K)
                cd[:rows, :K] = S8
                assert bool((cd == S8).all()), (rows, K, "a code byte outside [rows, K] changed")
                assert bool((sd[:5] == S32).all() and (sd[5 + rows:] == S32).all()), (rows, K, "a scale beside the rows changed")
                if is_grid:
                    assert torch.equal(rc.to(torch.int16), c) and torch.equal(rs, C.pow2(e)), (rows, K, "grid rows are their own codes")
