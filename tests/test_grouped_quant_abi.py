"""CPU: the grouped expert GEMVs over the int8 and NF4 decode copies (mp_gemv_grouped_w8_bf16, mp_gemv_grouped_w4_bf16) are declared in
include/medplib_hip.h, exported by the library and refuse bad arguments before any launch, each with its own name in the message; the two ops
wrappers refuse CPU tensors; and the mode table names grouped ops that exist."""
import ctypes
import os

import pytest
import torch

from medplib_amd import _lib

NEW = ("mp_gemv_grouped_w8_bf16", "mp_gemv_grouped_w4_bf16")
P = 4096                      # any non-null address: every refusal below comes before a launch
SHAPE, ARG = -1, -5           # MP_ERR_SHAPE, MP_ERR_ARG


def test_header_declares_and_library_exports_the_grouped_quantised_entry_points():
    protos = _lib.parse_header()
    assert all(n in protos for n in NEW), [n for n in NEW if n not in protos]
    if not os.path.exists(_lib.LIB_PATH):
        from medplib_amd import build
        build.build(verbose=False)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(dll, n) for n in NEW)


def _w8(L, M=2, N=256, K=512, E=2, act=0, residual=None, x=P, codes=P, scale=P, y=P, w_index=P):
    return L.raw("mp_gemv_grouped_w8_bf16")(x, K, codes, K, N * K, scale, N, y, N, residual, N, w_index, None, None, M, N, K, E, act, None)


def _w4(L, M=2, N=256, K=512, E=2, act=0, residual=None, x=P, codes=P, absmax=P, y=P, w_index=P, ldw=None, stride_w=None, lda=None):
    ldw = K // 2 if ldw is None else ldw
    lda = K // 64 if lda is None else lda
    return L.raw("mp_gemv_grouped_w4_bf16")(x, K, codes, ldw, N * ldw if stride_w is None else stride_w, absmax, lda, N * lda, y, N, residual, N,
                                            w_index, None, None, M, N, K, E, act, None)


@pytest.mark.parametrize("name,call,kmult,operands", [("mp_gemv_grouped_w8_bf16", _w8, 16, ("x", "codes", "scale", "y", "w_index")),
                                                      ("mp_gemv_grouped_w4_bf16", _w4, 64, ("x", "codes", "absmax", "y", "w_index"))])
def test_grouped_quantised_gemvs_refuse_before_any_launch(name, call, kmult, operands):
    L = _lib.lib()

    def refused(code, words, **kw):
        assert call(L, **kw) == code, (kw, L.last_error())
        assert name + ":" in L.last_error() and words in L.last_error(), (kw, L.last_error())

    for M in (0, 9):
        refused(SHAPE, "M <= 8", M=M)
    for E in (0, -1):
        refused(SHAPE, "E >= 1", E=E)
    for K in (kmult // 2, kmult + 8, 3 * kmult + kmult // 2):
        kw = dict(K=K) if kmult == 16 else dict(K=K, ldw=512, lda=64)
        refused(SHAPE, f"K % {kmult}", **kw)
    for act in (1, 2, 3, 4, 6, -1):                            # RELU, GELU, QUICK_GELU, SILU, ROPE_QK, nonsense
        refused(ARG, "only NONE / SWIGLU_PAIR", act=act)
    refused(ARG, "N % 64", act=5, N=1000)
    refused(ARG, "no residual", act=5, N=256, residual=P)
    for null in operands:
        refused(ARG, "null operand", **{null: None})
    refused(ARG, "w_index is required", w_index=None)


def test_grouped_w4_keeps_the_byte_stride_rules_of_the_indexed_form():
    L = _lib.lib()
    assert _w4(L, ldw=264) == SHAPE and "mp_gemv_grouped_w4_bf16: ldw_bytes % 16" in L.last_error()     # a row stride the 16-byte loads cannot take
    assert _w4(L, ldw=240) == SHAPE and "ldw_bytes" in L.last_error()                                    # rows that overlap
    assert _w4(L, stride_w=256 * 256 + 8) == SHAPE and "strideW_bytes % 16" in L.last_error()
    assert _w4(L, lda=7) == SHAPE and "mp_gemv_grouped_w4_bf16: lda >= K / 64" in L.last_error()


def test_grouped_quantised_ops_refuse_cpu_tensors():
    from medplib_amd import ops
    x, idx = torch.zeros(2, 64, dtype=torch.bfloat16), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.gemv_grouped_w8(x, torch.zeros(2, 16, 64, dtype=torch.int8), torch.zeros(2, 16), idx)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.gemv_grouped_w4(x, torch.zeros(2, 16, 32, dtype=torch.uint8), torch.zeros(2, 16, 1), idx)


def test_mode_table_names_grouped_ops_that_exist():
    from medplib_amd import ops
    from medplib_amd.model.llama import DECODE_MODES, DecodeMode
    assert DecodeMode._fields[-1] == "gemv_grouped", "a new LAST field: positional uses of the earlier ones still hold"
    assert DECODE_MODES[8].gemv_grouped == "gemv_grouped_w8" and DECODE_MODES[4].gemv_grouped == "gemv_grouped_w4"
    for mode in DECODE_MODES.values():
        assert callable(getattr(ops, mode.gemv_grouped)) and callable(getattr(ops, mode.gemv))
