"""CPU: the device-side LoRA merge (mp_lora_merge_rows_bf16 and its table form) is declared in include/medplib_hip.h, exported by the
library, and refuses bad shapes and null operands before any launch; ops.lora_merge_rows has no CPU path (no GPU needed)."""
import ctypes
import os

import pytest
import torch

from medplib_amd import _lib, ops

NEW = ("mp_lora_merge_rows_bf16", "mp_lora_merge_rows_batched")
FAKE = 64            # a non-null, 16-byte aligned address: every call below returns before it would be dereferenced or launched


def test_header_declares_and_library_exports_the_merge_entry_points():
    protos = _lib.parse_header()
    assert all(n in protos for n in NEW), [n for n in NEW if n not in protos]
    assert [a for _, a in protos["mp_lora_merge_rows_bf16"][1]] == ["Wsrc", "ldsrc", "Wdst", "lddst", "a", "b", "rows", "r", "fin", "fout", "scaling",
                                                                   "stream"]
    assert [t for t, _ in protos["mp_lora_merge_rows_bf16"][1]] == ["const void*", "int64_t", "void*", "int64_t", "const float*", "const float*",
                                                                   "const int64_t*", "int", "int", "int", "float", "hipStream_t"]
    assert [a for _, a in protos["mp_lora_merge_rows_batched"][1]] == ["descs", "n", "stream"]
    if not os.path.exists(_lib.LIB_PATH):
        from medplib_amd import build
        build.build(verbose=False)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(dll, n) for n in NEW)


def _merge(L, src=FAKE, ldsrc=64, dst=FAKE, lddst=64, a=FAKE, b=FAKE, rows=FAKE, r=8, fin=64, fout=16):
    return L.raw("mp_lora_merge_rows_bf16")(src, ldsrc, dst, lddst, a, b, rows, r, fin, fout, 2.0, None)


@pytest.mark.parametrize("kw", [dict(r=0), dict(r=65), dict(fin=12, ldsrc=16, lddst=16), dict(ldsrc=12, fin=8), dict(lddst=12, fin=8),
                                dict(ldsrc=56), dict(fout=-1)])
def test_bad_shapes_are_refused_before_any_launch(kw):
    L = _lib.lib()
    assert _merge(L, **kw) == -1, kw
    assert "mp_lora_merge_rows_bf16" in L.last_error()


@pytest.mark.parametrize("null", ["src", "dst", "a", "b", "rows"])
def test_null_operands_are_refused_before_any_launch(null):
    L = _lib.lib()
    assert _merge(L, **{null: None}) == -5
    assert "mp_lora_merge_rows_bf16" in L.last_error() and "null" in L.last_error()


def test_nothing_to_do_returns_ok():
    L = _lib.lib()
    assert _merge(L, fout=0) == 0
    assert _merge(L, src=None, dst=None, a=None, b=None, rows=None, fout=0) == 0            # no rows: the operands are not looked at
    assert _merge(L, fout=0, r=65) == -1                                                    # ... the shape still is
    batched = L.raw("mp_lora_merge_rows_batched")
    assert batched(None, 0, None) == 0 and batched(FAKE, 0, None) == 0
    assert batched(None, 3, None) == -5 and "mp_lora_merge_rows_batched" in L.last_error()
    assert batched(FAKE, -1, None) == -1 and "mp_lora_merge_rows_batched" in L.last_error()


def test_ops_refuse_cpu_tensors():
    w = torch.zeros(16, 64, dtype=torch.bfloat16)
    a, b, rows = torch.zeros(8, 64), torch.zeros(16, 8), torch.arange(16)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.lora_merge_rows(w, w, a, b, rows, 2.0)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.lora_merge_table([(w, w, a, b, rows, 2.0)], "cpu")
    with pytest.raises(ValueError, match="no CPU path"):
        ops.lora_merge_rows_batched(torch.zeros(72, dtype=torch.uint8), 1)
