"""CPU: the segmented routing entry points are declared in include/medplib_hip.h, exported by the library, and refuse a violated limit on the
host before any launch (no GPU needed); the drivers carry the batched-prefill switch, off by default."""
import ctypes
import inspect
import types

import pytest

from medplib_amd import _lib

TOP1, TOP2 = "mp_moe_route_top1_segments", "mp_moe_route_top2_segments"


def test_header_declares_the_segmented_routing():
    protos = _lib.parse_header()
    assert [t for t, _ in protos[TOP1][1]] == ["const float*", "const int*", "const int*", "int", "int", "int", "int", "int*", "int*", "float*",
                                               "int*", "long long*", "float*", "int*", "int*", "long long*", "hipStream_t"]
    assert [t for t, _ in protos[TOP2][1]] == ["const float*", "const float*", "const int*", "const int*", "int", "int", "int", "int", "int*",
                                               "int*", "float*", "int*", "long long*", "float*", "int*", "long long*", "hipStream_t"]


def test_limits_are_refused_before_any_launch():
    L = _lib.lib()

    def call(name, lens, caps, n, stride, E, slab_rows, lens_null=False):
        lens_c, caps_c = (ctypes.c_int * 16)(*lens), (ctypes.c_int * 16)(*caps)
        seg = (None if lens_null else ctypes.cast(lens_c, ctypes.c_void_p), ctypes.cast(caps_c, ctypes.c_void_p), n, stride, E, slab_rows)
        dev = (None,) * (9 if name == TOP1 else 8)            # the device operands: checked after the limits, never reached by a bad shape
        head = (None,) if name == TOP1 else (None, None)
        return L.raw(name)(*head, *seg, *dev, None)

    for name, top_k in ((TOP1, 1), (TOP2, 2)):
        for lens, caps, n, stride, E, slab in (([], [], 0, 16, 2, 8), ([4] * 9, [2] * 9, 9, 16, 2, 18), ([16, 17], [8, 8], 2, 16, 2, 16),
                                               ([16, 0], [8, 8], 2, 16, 2, 16), ([16, 7], [8, 4], 2, 16, 2, 11), ([16, 7], [8, 4], 2, 16, 9, 12),
                                               ([16, 7], [40, 40], 2, 16, 2, 23 * top_k - 1)):
            assert call(name, lens, caps, n, stride, E, slab) == -1 and name in L.last_error(), (name, lens, caps)
        assert call(name, [16, 7], [8, 4], 2, 16, 2, 12, lens_null=True) == -5 and "null operand" in L.last_error()
        assert call(name, [16, 7], [8, 4], 2, 16, 2, 12) == -5 and "null operand" in L.last_error()      # limits kept: the operands are next


def test_the_switch_is_off_by_default():
    from medplib_amd import infer
    from medplib_amd.model.generation import GenerationMixin as M
    for fn in (M.generate_batch, M._generate_groups, M._stream_batch, M._decode_batch):
        assert inspect.signature(fn).parameters["batch_prefill"].default is False
    assert inspect.signature(M._prefill_batch).parameters["batched"].default is False
    assert inspect.signature(infer.run_vqa).parameters["prefill_batch"].default is False
    assert infer.parse_args([]).prefill_batch is False and infer.parse_args(["--prefill_batch"]).prefill_batch is True
    with pytest.raises(ValueError, match="--prefill_batch"):
        infer.run_vqa([], types.SimpleNamespace(eval=lambda: None), None, decode_batch=1, prefill_batch=True)
