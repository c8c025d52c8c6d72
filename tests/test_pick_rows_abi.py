"""CPU: the per-row pick (mp_pick_rows_f32) and the per-row draws (mp_gate_noise_rows_dev_f32) are declared in include/medplib_hip.h with the
documented argument types, exported by the library and refuse bad arguments before any launch; the ops wrappers, the model's batch entry
points and the worker's batch loops exist with the documented signatures."""
import ctypes
import inspect
import os

import pytest
import torch

from medplib_amd import _lib

PICK, DRAWS = "mp_pick_rows_f32", "mp_gate_noise_rows_dev_f32"


def test_header_declares_and_library_exports_both_entry_points():
    protos = _lib.parse_header()
    assert protos[PICK][0] == "int" and protos[DRAWS][0] == "int"
    assert [n for _, n in protos[PICK][1]] == ["logits", "ld", "rows", "cols", "inv_temperature", "top_k", "top_p", "u", "out", "err", "stream"]
    assert [t for t, _ in protos[PICK][1]] == ["const float*", "int64_t", "int64_t", "int", "const float*", "const int*", "const float*",
                                               "const float*", "int64_t*", "int*", "hipStream_t"]
    assert [n for _, n in protos[DRAWS][1]] == ["out", "rows", "seeds", "step_dev", "stream"]
    assert [t for t, _ in protos[DRAWS][1]] == ["float*", "int64_t", "const int64_t*", "const int*", "hipStream_t"]
    header = open(_lib.HEADER_PATH).read()
    assert "#define MP_POS_ERR_PICK 8" in header and "#define MP_POS_ERR_BEAM 4" in header
    if not os.path.exists(_lib.LIB_PATH):
        from medplib_amd import build
        build.build(verbose=False)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(dll, PICK) and hasattr(dll, DRAWS)


def test_pick_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    pick, draws = L.raw(PICK), L.raw(DRAWS)
    one = ctypes.c_void_p(16)                                     # (never dereferenced: a refused call launches nothing)
    ok = dict(ld=32000, rows=2, cols=32000)
    for change in (dict(cols=0), dict(cols=65537, ld=65537), dict(rows=-1), dict(ld=31999), dict(cols=-3)):
        a = dict(ok, **change)
        for ptr in (None, one):                                   # the shape is refused first, null operands or not
            assert pick(ptr, a["ld"], a["rows"], a["cols"], ptr, ptr, ptr, ptr, ptr, ptr, None) == -1, change
            assert PICK in L.last_error(), change
    assert pick(None, 32000, 2, 32000, None, None, None, None, None, None, None) == -5
    assert PICK in L.last_error() and "null operand" in L.last_error()
    for hole in range(7):                                         # any single null operand
        ptrs = [None if i == hole else one for i in range(7)]
        assert pick(ptrs[0], 32000, 2, 32000, *ptrs[1:], None) == -5, hole
        assert PICK in L.last_error()
    assert pick(None, 0, 0, 32000, None, None, None, None, None, None, None) == 0           # no rows: nothing to do
    assert pick(one, 5, 1, 32000, one, one, one, one, None, one, None) == -5               # (one row: ld is not read; the null is)
    assert draws(None, -1, None, None, None) == -1 and DRAWS in L.last_error()
    for hole in range(3):
        ptrs = [None if i == hole else one for i in range(3)]
        assert draws(ptrs[0], 4, ptrs[1], ptrs[2], None) == -5, hole
        assert DRAWS in L.last_error()
    assert draws(None, 0, None, None, None) == 0


def test_wrappers_exist_and_refuse_cpu_tensors():
    from medplib_amd import ops
    assert ops.POS_ERR_PICK == 8
    assert list(inspect.signature(ops.pick_rows).parameters) == ["logits", "u", "inv_temperature", "top_k", "top_p", "err"]
    assert list(inspect.signature(ops.sample_uniform_rows).parameters) == ["seeds", "step"]
    f, i = (lambda n: torch.zeros(n)), (lambda n: torch.zeros(n, dtype=torch.int32))
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.pick_rows(torch.zeros(2, 8), f(2), f(2), i(2), f(2), i(1))
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.sample_uniform_rows(torch.zeros(2, dtype=torch.int64), 3)


def test_model_and_worker_methods_have_the_documented_signatures():
    from medplib_amd.model import generation as G
    from model.serve import model_worker as MW

    def names(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.name != "self"]

    E = inspect.Parameter.empty
    assert names(G.GenerationMixin.generate_sample_batch) == [
        ("input_ids", E), ("images", None), ("attention_mask", None), ("max_new_tokens", 512), ("eos_token_id", 2), ("temperature", 1.0),
        ("top_k", 50), ("top_p", 1.0), ("sample_seed", None), ("batch_rows", 8), ("kwargs", E)]
    assert names(G.GenerationMixin.generate_stream_batch) == [("requests", E), ("stream_interval", 1), ("eos_token_id", 2), ("debug", None)]
    r = G.StreamRequest(input_ids=[[1, 2]], images_clip=None)
    assert (r.images, r.resize_list, r.original_size_list, r.region_masks, r.valid_region_masks_bool) == (None, None, None, (), ())
    assert (r.temperature, r.top_p, r.top_k, r.apply_top_p) == (1.0, 1.0, 0, False)
    assert (r.max_new_tokens, r.stop_token_id, r.sample_seed, r.stop_check) == (256, None, 0, None)
    with pytest.raises(Exception):                                 # frozen
        r.temperature = 2.0
    assert G._RowsPick.needs_step is True
    assert names(MW.ModelWorker.generate_stream_batch) == [("params_list", E)]
    assert names(MW.ModelWorker.generate_stream_gate_batch) == [("params_list", E)]
    assert names(MW.ModelWorker.generate_stream) == [("params", E)] and names(MW.ModelWorker.generate_stream_gate) == [("params", E)]
