"""The three kernels under generate_batch, each against the entry point it is the per-row twin of, bit for bit: RoPE + KV append at a position
per row (ops.decode_rope_append_rows against ops.decode_rope_append on the row slices), single-query attention with a key count per row
(ops.attention_decode_rows against ops.attention with that row's count) and the grouped expert GEMV (ops.gemv_grouped against ops.gemv with
the same w_index).  Outputs that must stay untouched are pre-filled with a sentinel."""
import pytest
import torch

from medplib_amd import ops
from medplib_amd._lib import MedplibError, lib

pytestmark = pytest.mark.gpu

SENTINEL = -1984.0


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _randn(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------------- RoPE + append
def _rope_tables(rows, D, dev):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    f = torch.outer(torch.arange(rows, dtype=torch.float32), inv)
    return f.cos().contiguous().to(dev), f.sin().contiguous().to(dev)


@pytest.mark.parametrize("D", [64, 128])
def test_rope_append_rows_equals_the_one_position_entry_per_row(dev, D):
    B, H, ROWS = 3, 2, 40
    g = torch.Generator().manual_seed(100 + D)
    cos, sin = _rope_tables(ROWS, D, dev)
    qkv0 = _randn(g, B, 3 * H * D).to(dev)

    def fresh():
        return (qkv0.clone(), torch.full((B, ROWS, H, D), SENTINEL, dtype=torch.bfloat16, device=dev),
                torch.full((B, ROWS, H, D), SENTINEL, dtype=torch.bfloat16, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))

    def twin(pos):
        qkv, ck, cv, err = fresh()
        for b, p in enumerate(pos):
            ops.decode_rope_append(qkv[b:b + 1], cos, sin, ck[b:b + 1], cv[b:b + 1], torch.tensor([p], dtype=torch.int32, device=dev), H, D, err=err)
        return qkv, ck, cv, int(err[0])

    for pos in ([0, 17, 39], [3, 40, -1]):
        qkv, ck, cv, err = fresh()
        ops.decode_rope_append_rows(qkv, cos, sin, ck, cv, torch.tensor(pos, dtype=torch.int32, device=dev), H, D, err=err)
        r_qkv, r_ck, r_cv, r_err = twin(pos)
        assert _same(qkv, r_qkv) and _same(ck, r_ck) and _same(cv, r_cv), f"D={D} pos={pos}"
        assert int(err[0]) == r_err, f"D={D} pos={pos}: error word {int(err[0])}, the twin's {r_err}"
        for b, p in enumerate(pos):
            if 0 <= p < ROWS:          # the row was written at its own position, and nowhere else
                assert not bool((ck[b, p] == SENTINEL).any()) and _same(cv[b, p].reshape(-1), qkv0[b, 2 * H * D:])
                assert _same(qkv[b, :H * D], qkv0[b, :H * D]) == (p == 0)          # (position 0 rotates by nothing)
                rest = torch.ones(ROWS, dtype=torch.bool); rest[p] = False
                assert bool((ck[b][rest.to(dev)] == SENTINEL).all()) and bool((cv[b][rest.to(dev)] == SENTINEL).all())
            else:                      # out of range: nothing written, q included
                assert bool((ck[b] == SENTINEL).all()) and bool((cv[b] == SENTINEL).all()) and _same(qkv[b], qkv0[b])
    assert r_err != 0                  # (the second set has positions past the table and below 0)
    with pytest.raises(AssertionError):
        ops.decode_rope_append_rows(qkv0.clone(), cos, sin, ck, cv, torch.zeros(1, dtype=torch.int32, device=dev), H, D)


# ---------------------------------------------------------------------------------------------------------------------- attention rows
def _decode_splits(BH, Sk):
    """launch_attn_decode's split count with the workspace registered (as tests/test_gpu_attention_edges.py restates it)."""
    ns = min(16, 256 // BH) if BH <= 256 else 1
    while (Sk + ns - 1) // ns + 64 > 2048:
        ns += 1
    return ns


def _attention_rows_case(dev, D, cache, key_sets, tag):
    B, H = 3, 2
    g = torch.Generator().manual_seed(200 + D + cache)
    qkv = _randn(g, B, 1, 3, H, D).to(dev)
    q = qkv[:, :, 0]
    k, v = _randn(g, B, cache, H, D).to(dev), _randn(g, B, cache, H, D).to(dev)
    for keys in key_sets:
        out = ops.attention_decode_rows(q, k, v, torch.tensor(keys, dtype=torch.int32, device=dev))
        again = ops.attention_decode_rows(q, k, v, torch.tensor(keys, dtype=torch.int32, device=dev))
        assert out.shape == (B, 1, H * D) and _same(out, again), f"{tag} D={D} keys={keys}: the second call differs"
        for b, n in enumerate(keys):
            ref = ops.attention(q, k, v, causal=False, sk_dev=torch.tensor([n], dtype=torch.int32, device=dev))
            assert _same(out[b], ref[b]), f"{tag} D={D} keys={keys}: row {b} differs from attention(sk_dev=[{n}])"
        assert not _same(out[0], out[2])


@pytest.mark.parametrize("D", [128, 64])
def test_attention_rows_equal_attention_at_each_rows_count(dev, D):
    ns = _decode_splits(3 * 2, 200)
    sets = ([1, 64, 200], [16 * ns, 16 * ns + 1, 199], [16, 17, 31])
    _attention_rows_case(dev, D, 200, sets, f"workspace (NS={ns})")
    # without the split workspace: one split (the kernel normalises itself), and a cache too long for one split takes the tiled kernel row by row
    ops._ensure_gemm_workspace(dev)
    key = dev.index or 0
    ws, tickets = ops._GEMM_WS[key]
    lib().call("mp_gemm_set_workspace", None, 0, None, 0)
    try:
        _attention_rows_case(dev, D, 200, sets, "no workspace, NS=1")
        _attention_rows_case(dev, D, 2100, ([1, 1985, 2100],), "no workspace, tiled fallback")
    finally:
        lib().call("mp_gemm_set_workspace", ws.data_ptr(), ws.numel(), tickets.data_ptr(), tickets.numel())
    _attention_rows_case(dev, D, 200, sets[:1], "workspace again")


def test_attention_rows_argument_checks(dev):
    q = torch.zeros((2, 1, 2, 64), dtype=torch.bfloat16, device=dev)
    k = torch.zeros((2, 8, 2, 64), dtype=torch.bfloat16, device=dev)
    with pytest.raises(AssertionError):
        ops.attention_decode_rows(q, k, k, torch.ones(1, dtype=torch.int32, device=dev))
    with pytest.raises(TypeError):
        ops.attention_decode_rows(q, k, k, torch.ones(2, dtype=torch.int64, device=dev))


# ---------------------------------------------------------------------------------------------------------------------- grouped GEMV
E = 4
#            w_index                      row_keep (None: every row kept)
ROW_SETS = (([2], None),                                                    # M = 1
            ([1] * 8, None),                                                # one expert, two passes of four
            ([0, 1, 0, 0, 0], None),                                        # experts 2 and 3 named by nobody
            ([0, 3, 0, 3, 0, 0], [0, 0, -1, 1, 1, 2]),                      # a drop in the middle of a group
            ([0, 1, 0, 0, 0], [-1] * 5),                                    # every row dropped
            ([3, 0, 3, 2, 0, 3, 3, 2], [0, 0, 1, -1, 1, 2, 3, 0]))          # a full pass, a pair, a lone row and a drop


def _grouped_case(dev, w, N, K, act, seed):
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
            ref = ops.gemv(x, w, residual=residual, act=act, w_index=w_index, row_scale=row_scale, row_keep=row_keep)
            buf = torch.full((M + 1, cols + 1), SENTINEL, dtype=torch.bfloat16, device=dev)        # a guard column and a guard row
            ops.gemv_grouped(x, w, w_index, residual=residual, act=act, row_scale=row_scale, row_keep=row_keep, out=buf)
            tag = f"N={N} K={K} act={act} idx={idx} keep={keep} scale={with_scale} residual={with_res}"
            assert bool((buf[M] == SENTINEL).all()) and bool((buf[:, cols] == SENTINEL).all()), tag + ": wrote beyond M or N"
            got = buf[:M, :cols]
            for m in kept:
                assert _same(got[m], ref[m]), f"{tag}: row {m} differs from gemv(w_index=...) by {float((got[m].float() - ref[m].float()).abs().max())}"
            for m in dropped:
                if act == ops.ACT_SWIGLU_PAIR:
                    assert bool((got[m] == SENTINEL).all()), f"{tag}: dropped row {m} was written"
                else:                  # gv_store_dropped: the residual's own bits, +0 without one
                    assert _same(got[m], ref[m]) and _same(got[m], residual[m] if with_res else torch.zeros_like(got[m])), f"{tag}: dropped row {m}"
            if kept:
                assert bool((got[kept[0]] != SENTINEL).any())
            free = ops.gemv_grouped(x, w, w_index, residual=residual, act=act, row_scale=row_scale, row_keep=row_keep)      # (its own output)
            assert free.shape == (M, cols) and all(_same(free[m], ref[m]) for m in kept)


@pytest.mark.parametrize("K", [8, 520, 2568])          # tail only; one step + tail; a four-step trip + one step + tail
@pytest.mark.parametrize("N", [64, 192])
def test_grouped_gemv_swiglu_form_equals_the_indexed_form(dev, N, K):
    w = _randn(torch.Generator().manual_seed(N + K), E, N, K, scale=0.05).to(dev)
    _grouped_case(dev, w, N, K, ops.ACT_SWIGLU_PAIR, 300 + N + K)
    _grouped_case(dev, w, N, K, ops.ACT_NONE, 301 + N + K)              # the plain wave-per-four-rows form (K < 4096: no K split)


@pytest.mark.parametrize("K", [4096, 4104, 11008])
@pytest.mark.parametrize("N", [4, 20, 4096])
def test_grouped_gemv_ksplit_form_equals_the_indexed_form(dev, N, K):
    w = (torch.randn((E, N, K), generator=torch.Generator(device=dev).manual_seed(N + K), device=dev, dtype=torch.float32) * 0.05).to(torch.bfloat16)
    _grouped_case(dev, w, N, K, ops.ACT_NONE, 400 + N + K)


def test_grouped_gemv_stores_a_row_with_an_expert_out_of_range_as_dropped(dev):
    """A w_index outside [0, E) reads no weights: the row is stored as a capacity-dropped one."""
    g = torch.Generator().manual_seed(5)
    w, x, res = _randn(g, E, 20, 520, scale=0.05).to(dev), _randn(g, 3, 520).to(dev), _randn(g, 3, 20).to(dev)
    out = ops.gemv_grouped(x, w, torch.tensor([1, E, -1], dtype=torch.int32, device=dev), residual=res)
    ref = ops.gemv(x[:1], w, residual=res[:1], w_index=torch.tensor([1], dtype=torch.int32, device=dev))
    assert _same(out[0], ref[0]) and _same(out[1:], res[1:])


def test_grouped_gemv_argument_checks(dev):
    w = torch.zeros((E, 64, 16), dtype=torch.bfloat16, device=dev)
    x = torch.zeros((9, 16), dtype=torch.bfloat16, device=dev)
    with pytest.raises(MedplibError):              # M <= 8
        ops.gemv_grouped(x, w, torch.zeros(9, dtype=torch.int32, device=dev))
    with pytest.raises(MedplibError):              # only NONE / SWIGLU_PAIR
        ops.gemv_grouped(x[:2], w, torch.zeros(2, dtype=torch.int32, device=dev), act=ops.ACT_RELU)
    with pytest.raises(TypeError):
        ops.gemv_grouped(x[:2], w, torch.zeros(2, dtype=torch.int64, device=dev))
    with pytest.raises(AssertionError):            # a 2-D weight is the shared form's
        ops.gemv_grouped(x[:2], w[0], torch.zeros(2, dtype=torch.int32, device=dev))
