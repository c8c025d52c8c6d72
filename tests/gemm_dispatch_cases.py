"""Shared by tests/test_gpu_gemm_dispatch_table.py and scripts/make_gemm_dispatch_table.py: how a row of
tests/golden/gemm_dispatch_table.json (one bf16 GEMM call: C entry point, sizes, epilogue, tile policy, stream) is issued again, and the
hand-written rows the table holds beside the calls recorded from the product.

A row describes what the HOST selection looks at; the operands are zeros and every device-side row count is 0 (the selection cannot see
them), so the batched replays cost next to nothing."""
import contextlib

import torch

FIELDS = ("entry", "M", "N", "K", "batch", "act", "bias", "residual", "out", "alpha", "m_dev", "a_rows", "c_rows", "lda", "ldc", "seq", "pos",
          "policy", "stream")


def row(entry, M, N, K, batch=1, act=0, bias=False, residual=False, out="bf16", alpha=1.0, m_dev=False, a_rows=False, c_rows=False, lda=None,
        ldc=None, seq=0, pos=0, policy=-1, stream="primary"):
    n_out = N // 2 if act == 5 else N
    return {"entry": entry, "M": M, "N": N, "K": K, "batch": batch, "act": act, "bias": bias, "residual": residual, "out": out, "alpha": alpha,
            "m_dev": m_dev, "a_rows": a_rows, "c_rows": c_rows, "lda": K if lda is None else lda, "ldc": n_out if ldc is None else ldc, "seq": seq,
            "pos": pos, "policy": policy, "stream": stream}


def key(r):
    return tuple(r[f] for f in FIELDS)


def hand_rows():
    """The shapes of the selection tests in tests/test_gpu_trunk_kernels.py, every entry point under tile policies -1, 0 and 2, the small and
    the many-batch calls that stay on 128x128 tiles, and calls on a registered side stream."""
    rows = []
    NT, ROPE, KEEP = "mp_gemm_bf16_nt", "mp_gemm_qkv_rope_bounded_bf16", "mp_gemm_swiglu_keep_bf16"
    for (M, N, K) in [(4096, 4096, 512), (5112, 4096, 1024), (1100, 512, 256), (4616, 4096, 1024)]:
        for kw in ({}, {"residual": True}, {"alpha": 0.5}, {"bias": True, "act": 3, "residual": True}):
            rows += [row(NT, M, N, K, policy=p, **kw) for p in (2, 0)]
    rows += [row(NT, 4616, 4096, 1024, act=a, policy=p) for a in (2, 4, 1) for p in (2, 0)]
    rows += [row(ROPE, 4096, 3072, 512, act=6, seq=512, pos=2, policy=p) for p in (2, 0)]
    rows += [row(NT, 5112, N, 4096, policy=1) for N in (4096, 12288, 22016)] + [row(NT, 2304, 4096, 4096, policy=1)]
    rows += [row(NT, M, 4096, 11008, bias=True, residual=True, policy=p) for M in (2556, 2241, 1917) for p in (-1, 0)]
    for p in (-1, 0, 2):
        rows += [row(NT, 5112, 4096, 4096, policy=p), row(NT, 5112, 4096, 4096, out="f32", policy=p), row(NT, 5112, 22016, 4096, act=5, policy=p),
                 row(NT, 64, 4096, 4096, policy=p), row(NT, 1024, 1024, 4096, m_dev=True, policy=p),
                 row(ROPE, 5112, 12288, 4096, act=6, seq=639, policy=p), row("mp_gemm_qkv_rope_bf16", 5112, 12288, 4096, act=6, seq=639, policy=p),
                 row(ROPE, 512, 12288, 4096, act=6, seq=64, policy=p),
                 row("mp_gemm_qkv_rope_scaled_bounded_bf16", 5112, 12288, 4096, act=6, seq=639, policy=p),
                 row("mp_gemm_qkv_rope_scaled_bf16", 5112, 12288, 4096, act=6, seq=639, policy=p),
                 row(KEEP, 5112, 22016, 4096, act=5, policy=p), row(KEEP, 640, 22016, 4096, act=5, policy=p),
                 row("mp_gemm_bf16_nt_batched", 2816, 8192, 4096, batch=2, m_dev=True, policy=p),
                 row("mp_gemm_bf16_nt_batched", 2816, 4096, 1024, batch=2, m_dev=True, bias=True, act=2, policy=p),
                 row("mp_gemm_bf16_nt_batched", 128, 256, 64, batch=16, out="f32", policy=p),
                 row("mp_gemm_bf16_nt_batched_res", 2816, 4096, 4096, batch=2, residual=True, m_dev=True, policy=p),
                 row("mp_gemm_bf16_nt_batched_res", 256, 512, 64, batch=2, residual=True, policy=p),
                 row("mp_gemm_bf16_nt_batched_rows", 2816, 22016, 4096, batch=2, act=5, m_dev=True, a_rows=True, policy=p),
                 row("mp_gemm_bf16_nt_batched_rows", 2816, 4096, 11008, batch=2, residual=True, m_dev=True, c_rows=True, policy=p),
                 row("mp_gemm_bf16_nt_batched_rows", 2816, 4096, 4096, batch=2, m_dev=True, policy=p),
                 row("mp_gemm_bf16_nt_batched_rows", 256, 512, 128, batch=2, m_dev=True, a_rows=True, policy=p),
                 row("mp_gemm_bf16_nt_batched_rows_scaled", 2816, 22016, 4096, batch=2, act=5, m_dev=True, a_rows=True, policy=p)]
    # a registered side stream: the towers' whole-tile policy, and the default policy where the sub-wave split is the primary stream's alone
    rows += [row(NT, 4616, 1024, 4096, bias=True, residual=True, policy=3, stream="side"), row(NT, 512, 256, 6912, policy=3, stream="side"),
             row(NT, 2556, 4096, 11008, stream="side"), row(NT, 5112, 4096, 4096, stream="side"), row(NT, 64, 4096, 4096, stream="side"),
             row(ROPE, 5112, 12288, 4096, act=6, seq=639, stream="side"), row(KEEP, 5112, 22016, 4096, act=5, stream="side")]
    return rows


def _mat(dev, rows, cols, ld=None, dtype=torch.bfloat16):
    return torch.zeros((rows, max(cols, ld or cols)), dtype=dtype, device=dev)[:, :cols]


def replay(r, dev):
    """Issue the call `r` describes and return ops.gemm_last_kernel()."""
    from medplib_amd import ops
    from medplib_amd.ops import _p, _stream, lib
    e, M, N, K, E, act = r["entry"], r["M"], r["N"], r["K"], r["batch"], r["act"]
    bf, odt = torch.bfloat16, (torch.float32 if r["out"] == "f32" else torch.bfloat16)
    n_out = N // 2 if act == ops.ACT_SWIGLU_PAIR else N
    counts = torch.zeros(E, dtype=torch.int32, device=dev) if r["m_dev"] else None
    side = ops.side_stream(dev, "clip", with_gemm_workspace=True) if r["stream"] == "side" else None
    prev = ops._TILE_POLICY
    ops.gemm_tile_policy(r["policy"])
    try:
        with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
            if e == "mp_gemm_bf16_nt":
                ops.gemm(_mat(dev, M, K, r["lda"]), _mat(dev, N, K), bias=torch.zeros(N, device=dev) if r["bias"] else None,
                         residual=_mat(dev, M, n_out) if r["residual"] else None, act=act, out=_mat(dev, M, n_out, r["ldc"], odt), alpha=r["alpha"],
                         m_dev=counts)
            elif e == "mp_gemm_swiglu_keep_bf16":
                ops.gemm_swiglu_keep(_mat(dev, M, K, r["lda"]), _mat(dev, N, K))
            elif "qkv_rope" in e:
                rows_t = r["seq"] + r["pos"]
                cos_t, sin_t = torch.ones(rows_t, 64, device=dev), torch.zeros(rows_t, 64, device=dev)
                a, w, out = _mat(dev, M, K, r["lda"]), _mat(dev, N, K), _mat(dev, M, N, r["ldc"])
                scale = torch.ones(M, device=dev) if "scaled" in e else None
                if "bounded" in e:
                    ops.gemm_qkv_rope(a, w, cos_t, sin_t, r["seq"], N // 384, 128, pos_offset=r["pos"], out=out, row_scale=scale)
                else:               # the unbounded entry points have no wrapper of their own
                    ops._ensure_gemm_workspace(dev)
                    mid = (_p(scale),) if scale is not None else ()
                    lib().call(e, _p(a), a.stride(0), _p(w), w.stride(0), _p(out), out.stride(0), _p(cos_t), _p(sin_t), *mid, M, N, K, r["seq"], r["pos"], 128,
                               _stream())
            elif e == "mp_gemm_bf16_nt_batched":
                ops.gemm_batched(torch.zeros(E, M, K, dtype=bf, device=dev), torch.zeros(E, N, K, dtype=bf, device=dev),
                                 torch.zeros(E, M, n_out, dtype=odt, device=dev), m_dev=counts,
                                 bias=torch.zeros(E, N, device=dev) if r["bias"] else None, act=act)
            elif e == "mp_gemm_bf16_nt_batched_res":
                ops.gemm_batched_res(torch.zeros(E, M, K, dtype=bf, device=dev), torch.zeros(E, N, K, dtype=bf, device=dev),
                                     torch.zeros(E, M, N, dtype=bf, device=dev), torch.zeros(E, M, N, dtype=bf, device=dev), m_dev=counts)
            elif e in ("mp_gemm_bf16_nt_batched_rows", "mp_gemm_bf16_nt_batched_rows_scaled"):
                # shared matrices of M "tokens"; all row indices 0 (valid rows, and the zero counts keep the kernels from touching them)
                idx = torch.zeros(E * M, dtype=torch.int32, device=dev)
                a = _mat(dev, M, K, r["lda"]) if r["a_rows"] else torch.zeros(E, M, K, dtype=bf, device=dev)
                out = _mat(dev, M, n_out, r["ldc"]) if r["c_rows"] else torch.zeros(E, M, n_out, dtype=bf, device=dev)
                ops.gemm_batched_rows(a, torch.zeros(E, N, K, dtype=bf, device=dev), out, counts, a_rows=idx if r["a_rows"] else None,
                                      c_rows=idx if r["c_rows"] else None, c_scale=torch.ones(M, device=dev) if r["c_rows"] else None,
                                      residual=_mat(dev, M, N) if r["residual"] else None, act=act, rows_stride=M,
                                      a_row_scale=torch.ones(M, device=dev) if e.endswith("_scaled") else None)
            else:
                raise ValueError(e)
            tile = ops.gemm_last_kernel()
        torch.cuda.synchronize()
    finally:
        ops.gemm_tile_policy(prev)
    return tile
