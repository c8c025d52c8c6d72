"""The grouped expert GEMVs over the int8 and NF4 decode copies (ops.gemv_grouped_w8, ops.gemv_grouped_w4) against the indexed form of the same
weight type (ops.gemv_w8 / ops.gemv_w4 with the same w_index, row_scale, row_keep and residual), bit for bit, on copies made by
ops.quantize_rows_w8 / ops.quantize_blocks_nf4: the grouped section of tests/test_gpu_batch_kernels.py for the two quantised weight types, at
the smallest shapes that reach each loop edge of each form.  Outputs that must stay untouched are pre-filled with a sentinel."""
import pytest
import torch

from medplib_amd import ops

pytestmark = pytest.mark.gpu

SENTINEL = -1984.0
E = 4
#            w_index                      row_keep (None: every row kept)
ROW_SETS = (([2], None),                                                    # M = 1
            ([1] * 8, None),                                                # one expert, eight rows
            ([0, 1, 0, 0, 0], None),                                        # experts 2 and 3 named by nobody
            ([0, 3, 0, 3, 0, 0], [0, 0, -1, 1, 1, 2]),                      # a drop in the middle of a group
            ([0, 1, 0, 0, 0], [-1] * 5),                                    # every row dropped
            ([3, 0, 3, 2, 0, 3, 3, 2], [0, 0, 1, -1, 1, 2, 3, 0]))          # a full pass, a pair, a lone row and a drop
KINDS = ("w8", "w4")
_COPIES = {}


def _quantize(kind, w):
    return ops.quantize_rows_w8(w) if kind == "w8" else ops.quantize_blocks_nf4(w)


def _indexed(kind, x, copies, w_index, **kw):
    """The reference: the indexed form of the same weight type."""
    if kind == "w8":
        return ops.gemv_w8(x, *copies, w_index=w_index, **kw)
    return ops.gemv_w4(x, *copies, w_index=w_index, **kw)


def _grouped(kind, x, copies, w_index, **kw):
    if kind == "w8":
        return ops.gemv_grouped_w8(x, *copies, w_index, **kw)
    return ops.gemv_grouped_w4(x, *copies, w_index, **kw)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _randn(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


def _copies(dev, kind, N, K):
    """The quantised copies of E random [N, K] matrices, stacked: (codes, scale) / (codes, absmax).  Quantised expert by expert (the bf16
    source of one expert at a time), made once per shape and never written."""
    key = (kind, N, K)
    if key not in _COPIES:
        _COPIES.clear()                      # (one shape's copies at a time)
        g = torch.Generator(device=dev).manual_seed(N + K)
        parts = [_quantize(kind, (torch.randn((N, K), generator=g, device=dev, dtype=torch.float32) * 0.05).to(torch.bfloat16)) for _ in range(E)]
        _COPIES[key] = tuple(torch.stack([p[i] for p in parts]).contiguous() for i in range(2))
    return _COPIES[key]


def _grouped_case(dev, kind, N, K, act, seed):
    copies = _copies(dev, kind, N, K)
    g = torch.Generator().manual_seed(seed)
    cols = N // 2 if act == ops.ACT_SWIGLU_PAIR else N
    for idx, keep in ROW_SETS:
        M = len(idx)
        x = _randn(g, M, K).to(dev)
        w_index = torch.tensor(idx, dtype=torch.int32, device=dev)
        row_keep = None if keep is None else torch.tensor(keep, dtype=torch.int32, device=dev)
        kept = [m for m in range(M) if keep is None or keep[m] >= 0]
        dropped = [m for m in range(M) if m not in kept]
        variants = [(False, False)] if act == ops.ACT_SWIGLU_PAIR else [(False, False), (True, True), (True, False), (False, True)]
        for with_scale, with_res in variants:
            row_scale = (torch.rand(M, generator=g) + 0.25).to(dev) if with_scale else None
            residual = _randn(g, M, N).to(dev) if with_res else None
            ref = _indexed(kind, x, copies, w_index, residual=residual, act=act, row_scale=row_scale, row_keep=row_keep)
            buf = torch.full((M + 1, cols + 1), SENTINEL, dtype=torch.bfloat16, device=dev)        # a guard column and a guard row
            _grouped(kind, x, copies, w_index, residual=residual, act=act, row_scale=row_scale, row_keep=row_keep, out=buf)
            tag = f"{kind} N={N} K={K} act={act} idx={idx} keep={keep} scale={with_scale} residual={with_res}"
            assert bool((buf[M] == SENTINEL).all()) and bool((buf[:, cols] == SENTINEL).all()), tag + ": wrote beyond M or N"
            got = buf[:M, :cols]
            for m in kept:
                assert _same(got[m], ref[m]), f"{tag}: row {m} differs from the indexed form by {float((got[m].float() - ref[m].float()).abs().max())}"
            for m in dropped:
                if act == ops.ACT_SWIGLU_PAIR:
                    assert bool((got[m] == SENTINEL).all()), f"{tag}: dropped row {m} was written"
                else:                  # gv_store_dropped: the residual's own bits, +0 without one
                    assert _same(got[m], ref[m]) and _same(got[m], residual[m] if with_res else torch.zeros_like(got[m])), f"{tag}: dropped row {m}"
            if kept:
                assert bool((got[kept[0]] != SENTINEL).any())
            free = _grouped(kind, x, copies, w_index, residual=residual, act=act, row_scale=row_scale, row_keep=row_keep)      # (its own output)
            assert free.shape == (M, cols) and all(_same(free[m], ref[m]) for m in kept)


# int8: a wave step is 1024 elements (16 per lane).  One lane; one step + a ragged step; three steps + a ragged one.
@pytest.mark.parametrize("K", [16, 1040, 3088])
@pytest.mark.parametrize("N", [64, 192])
def test_w8_wave_forms_equal_the_indexed_form(dev, N, K):
    _grouped_case(dev, "w8", N, K, ops.ACT_SWIGLU_PAIR, 500 + N + K)
    _grouped_case(dev, "w8", N, K, ops.ACT_NONE, 501 + N + K)                # the plain wave-per-four-rows form (K < 4096: no K split)


# int8 K-split: a part's step is 1024 of every 4096.  One step per part; a ragged step in part 0 only; three steps in parts 0..2, two in part 3.
@pytest.mark.parametrize("N,K", [(N, K) for K in (4096, 4112, 11008) for N in (4, 20)] + [(4096, 4096)])
def test_w8_ksplit_form_equals_the_indexed_form(dev, N, K):
    _grouped_case(dev, "w8", N, K, ops.ACT_NONE, 600 + N + K)


# NF4 wave form: a step is 2048 elements (32 per lane, 16-byte loads).  Two lanes; one step + a tail; and for SwiGLU two steps + a tail at a K
# past the K-split threshold, which must stay in the wave form.
@pytest.mark.parametrize("K", [64, 2112, 4160])
@pytest.mark.parametrize("N", [64, 192])
def test_w4_wave_forms_equal_the_indexed_form(dev, N, K):
    _grouped_case(dev, "w4", N, K, ops.ACT_SWIGLU_PAIR, 700 + N + K)
    if K < 4096:
        _grouped_case(dev, "w4", N, K, ops.ACT_NONE, 701 + N + K)


# NF4 K-split: 8-byte loads, a part's step is 1024 of every 4096.
@pytest.mark.parametrize("N,K", [(N, K) for K in (4096, 4160, 11008) for N in (4, 20)] + [(4096, 4096)])
def test_w4_ksplit_form_equals_the_indexed_form(dev, N, K):
    _grouped_case(dev, "w4", N, K, ops.ACT_NONE, 800 + N + K)


@pytest.mark.parametrize("kind,K", [("w8", 1040), ("w8", 4112), ("w4", 2112), ("w4", 4160)])
def test_a_row_with_an_expert_out_of_range_is_stored_as_dropped(dev, kind, K):
    """A w_index outside [0, E) reads no weights: the plain forms store the row as a capacity-dropped one, the SwiGLU form leaves it unwritten."""
    g = torch.Generator().manual_seed(5 + K)
    x = _randn(g, 3, K).to(dev)
    one, bad = torch.tensor([1], dtype=torch.int32, device=dev), torch.tensor([1, E, -1], dtype=torch.int32, device=dev)
    copies, res = _copies(dev, kind, 20, K), _randn(g, 3, 20).to(dev)
    out = _grouped(kind, x, copies, bad, residual=res)
    assert _same(out[0], _indexed(kind, x[:1], copies, one, residual=res[:1])[0]) and _same(out[1:], res[1:])
    out = _grouped(kind, x, copies, bad)
    assert _same(out[0], _indexed(kind, x[:1], copies, one)[0]) and _same(out[1:], torch.zeros_like(out[1:]))
    copies = _copies(dev, kind, 64, K)
    buf = torch.full((3, 32), SENTINEL, dtype=torch.bfloat16, device=dev)
    _grouped(kind, x, copies, bad, act=ops.ACT_SWIGLU_PAIR, out=buf)
    assert _same(buf[0], _indexed(kind, x[:1], copies, one, act=ops.ACT_SWIGLU_PAIR)[0]) and bool((buf[1:] == SENTINEL).all())


@pytest.mark.parametrize("kind,N,K,act", [("w8", 64, 1040, ops.ACT_SWIGLU_PAIR), ("w8", 64, 1040, ops.ACT_NONE), ("w8", 20, 4112, ops.ACT_NONE),
                                          ("w4", 64, 2112, ops.ACT_SWIGLU_PAIR), ("w4", 64, 2112, ops.ACT_NONE), ("w4", 20, 4160, ops.ACT_NONE)])
def test_grouping_is_invisible(dev, kind, N, K, act):
    """A row's bits do not depend on the rows it shares a launch or a pass with: the last row set in another order, and every row alone."""
    copies = _copies(dev, kind, N, K)
    idx, keep = ROW_SETS[-1]
    M = len(idx)
    g = torch.Generator().manual_seed(900 + N + K)
    x = _randn(g, M, K).to(dev)
    plain = act == ops.ACT_NONE
    row_scale = (torch.rand(M, generator=g) + 0.25).to(dev) if plain else None
    residual = _randn(g, M, N).to(dev) if plain else None
    w_index, row_keep = torch.tensor(idx, dtype=torch.int32, device=dev), torch.tensor(keep, dtype=torch.int32, device=dev)
    kept = [m for m in range(M) if keep[m] >= 0]

    def run(rows):
        r = torch.tensor(rows, device=dev)
        sub = lambda t: None if t is None else t[r].contiguous()           # noqa: E731
        return _grouped(kind, x[r].contiguous(), copies, w_index[r].contiguous(), residual=sub(residual), act=act, row_scale=sub(row_scale), row_keep=sub(row_keep))

    base = run(list(range(M)))
    for perm in ([7, 6, 5, 4, 3, 2, 1, 0], [2, 5, 1, 7, 0, 3, 6, 4]):
        out = run(perm)
        for j, m in enumerate(perm):
            if m in kept:
                assert _same(out[j], base[m]), (perm, m)
    for m in kept:
        assert _same(run([m])[0], base[m]), m
