"""CPU: the 8-bit decode-weight entry points (row-wise absmax quantiser, int8-weight GEMV) are declared in include/medplib_hip.h, exported by
the library and refuse bad arguments before any launch; ops.gemv_w8 refuses CPU tensors; the worker's --load-8bit passes its placement check."""
import ctypes
import os

import pytest
import torch

from medplib_amd import _lib

NEW = ("mp_quantize_rows_w8_bf16", "mp_gemv_w8_bf16")
P = 4096                      # any non-null address: every refusal below comes before a launch


def test_header_declares_and_library_exports_the_w8_entry_points():
    protos = _lib.parse_header()
    assert all(n in protos for n in NEW), [n for n in NEW if n not in protos]
    if not os.path.exists(_lib.LIB_PATH):
        from medplib_amd import build
        build.build(verbose=False)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(dll, n) for n in NEW)


def _gemv(L, M=1, N=256, K=512, act=0, bias=None, residual=None, x=P, W=P, scale=P, y=P, out_dtype=0):
    return L.raw("mp_gemv_w8_bf16")(x, K, W, K, 0, scale, 0, y, N, bias, residual, N, None, None, None, M, N, K, act, out_dtype, 1.0, None)


def test_gemv_w8_refuses_before_any_launch():
    L = _lib.lib()
    for M in (0, 9):
        assert _gemv(L, M=M) == -1 and "mp_gemv_w8_bf16" in L.last_error() and "M <= 8" in L.last_error()
    assert _gemv(L, K=24) == -1 and "K % 16" in L.last_error()
    assert _gemv(L, bias=P) == -5 and "bias" in L.last_error()
    for act in (1, 2, 3, 4, 6, -1):                            # RELU, GELU, QUICK_GELU, SILU, ROPE_QK, nonsense
        assert _gemv(L, act=act) == -5 and "NONE or SWIGLU_PAIR" in L.last_error()
    assert _gemv(L, act=5, N=1000) == -5 and "N % 64" in L.last_error()
    assert _gemv(L, act=5, N=256, residual=P) == -5             # SWIGLU_PAIR takes no residual, as in mp_gemv_bf16
    assert _gemv(L, out_dtype=7) == -2
    for null in ("x", "W", "scale", "y"):
        assert _gemv(L, **{null: None}) == -5 and "null operand" in L.last_error()


def test_quantizer_refuses_before_any_launch():
    L = _lib.lib()
    q = L.raw("mp_quantize_rows_w8_bf16")
    assert q(P, 512, 0, 512, P, 512, P, None) == -1 and "mp_quantize_rows_w8_bf16" in L.last_error()      # no rows
    assert q(P, 24, 4, 24, P, 24, P, None) == -1 and "K % 16" in L.last_error()
    assert q(P, 256, 4, 512, P, 512, P, None) == -1            # ldw < K
    for args in ((None, 512, 4, 512, P, 512, P, None), (P, 512, 4, 512, None, 512, P, None), (P, 512, 4, 512, P, 512, None, None)):
        assert q(*args) == -5 and "null operand" in L.last_error()


def test_ops_w8_refuse_cpu_tensors():
    from medplib_amd import ops
    x = torch.zeros(1, 32, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.gemv_w8(x, torch.zeros(16, 32, dtype=torch.int8), torch.zeros(16))
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.quantize_rows_w8(torch.zeros(16, 32, dtype=torch.bfloat16))


def test_worker_accepts_load_8bit_and_still_refuses_the_other_loads():
    from model.serve import model_worker as MW
    base = ["--model-path", "checkpoints/tiny", "--device_map", "cuda"]
    args = MW.parse_args(base + ["--load-8bit"])
    assert args.load_8bit
    MW.check_placement(args)
    for flag in ("--load-4bit", "--load-fp16"):
        with pytest.raises(ValueError, match="bf16"):
            MW.check_placement(MW.parse_args(base + [flag]))
    with pytest.raises(ValueError, match="bf16"):
        MW.check_placement(MW.parse_args(base + ["--precision", "int8"]))
    with pytest.raises(NotImplementedError, match="device_map"):
        MW.check_placement(MW.parse_args(["--model-path", "checkpoints/tiny", "--load-8bit"]))
