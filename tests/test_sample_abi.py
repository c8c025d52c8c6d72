"""CPU: the sampling pick (mp_sample_rows_f32) is declared in include/medplib_hip.h, exported by the library and refuses bad arguments before
any launch; ops.sample_rows refuses CPU tensors; the serving worker's face parses the reference's command line (no GPU needed)."""
import ctypes
import os

import pytest
import torch

from medplib_amd import _lib


def test_header_declares_and_library_exports_the_sampling_pick():
    protos = _lib.parse_header()
    assert "mp_sample_rows_f32" in protos
    assert [t for t, _ in protos["mp_sample_rows_f32"][1]] == ["const float*", "int64_t", "int64_t", "int", "float", "const float*", "int64_t*",
                                                               "hipStream_t"]
    if not os.path.exists(_lib.LIB_PATH):
        from medplib_amd import build
        build.build(verbose=False)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mp_sample_rows_f32")


def test_sampling_pick_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    f = L.raw("mp_sample_rows_f32")
    for cols, inv_t in ((0, 1.0), (-3, 1.0), (65537, 1.0), (32000, 0.0), (32000, -1.0), (32000, float("inf")), (32000, float("nan"))):
        assert f(None, cols, 1, cols, inv_t, None, None, None) == -1, (cols, inv_t)
        assert "mp_sample_rows_f32" in L.last_error()
    assert f(None, 32000, 1, 32000, 1.0, None, None, None) == -5 and "null operand" in L.last_error()      # the operands are checked next
    assert f(None, 32000, 0, 32000, 1.0, None, None, None) == 0                                             # no rows: nothing to do


def test_sample_rows_refuses_cpu_tensors():
    from medplib_amd import ops
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.sample_rows(torch.zeros(1, 8), torch.zeros(1), 1.0)


def test_worker_face_parses_the_reference_command_line():
    from model.serve import model_worker as MW
    names = [n for n, _, _ in MW.FLAG_TABLE]
    assert len(names) == len(set(names))
    for n in ("model-path", "model-name", "vision_pretrained", "stream-interval", "limit-model-concurrency", "add_region_feature", "image_w",
              "image_h", "precision", "device_map"):
        assert n in names, n
    args = MW.parse_args(["--host", "0.0.0.0", "--controller-address", "http://localhost:10000", "--port", "40000", "--worker-address",
                          "http://localhost:40000", "--model-path", "checkpoints/xxx", "--multi-modal", "--add_region_feature"])
    assert args.model_path == "checkpoints/xxx" and args.multi_modal and args.add_region_feature and args.stream_interval == 1
    assert args.limit_model_concurrency == 5 and args.image_w == 336 and args.image_h == 336 and args.model_name == "medplib"
    assert args.precision == "bf16" and args.device_map == "cpu"
    with pytest.raises(NotImplementedError, match="device_map"):
        MW.check_placement(args)                                  # the reference's default placement is the CPU: refused
    args.device_map = "cuda"
    MW.check_placement(args)
    args.precision = "fp16"
    with pytest.raises(ValueError, match="bf16"):
        MW.check_placement(args)
    assert MW.encode_sparse([[0, 1], [1, 0]]) == [[0, 1], [1, 0]]
