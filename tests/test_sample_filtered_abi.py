"""CPU: the truncated sampling pick (mp_sample_filtered_rows_f32) is declared in include/medplib_hip.h, exported by the library and refuses
bad arguments before any launch; ops.sample_rows_filtered refuses CPU tensors; the worker and the vqa walk parse their flags; and the
float64 rule the GPU tests hold the kernel to (tests/sample_filter_cases.py) keeps what HF's Temperature -> TopK -> TopP warper chain keeps."""
import ctypes
import os

import numpy as np
import pytest
import torch

from medplib_amd import _lib
from sample_filter_cases import kept_rule

NAME = "mp_sample_filtered_rows_f32"


def test_header_declares_and_library_exports_the_filtered_pick():
    protos = _lib.parse_header()
    assert NAME in protos and protos[NAME][0] == "int"
    assert [t for t, _ in protos[NAME][1]] == ["const float*", "int64_t", "int64_t", "int", "float", "int", "float", "const float*", "int64_t*",
                                               "int*", "float*", "hipStream_t"]
    assert [n for _, n in protos[NAME][1]] == ["logits", "ld", "rows", "cols", "inv_temperature", "top_k", "top_p", "u", "out", "kept", "cut",
                                               "stream"]
    header = open(_lib.HEADER_PATH).read()
    comment = header[:header.index("int " + NAME)].rsplit("/*", 1)[1]
    for word in ("TemperatureLogitsWarper", "TopKLogitsWarper", "TopPLogitsWarper", "vqa_infer.py:430-442"):
        assert word in comment, word
    if not os.path.exists(_lib.LIB_PATH):
        from medplib_amd import build
        build.build(verbose=False)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)


def test_filtered_pick_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    f = L.raw(NAME)
    inf, nan = float("inf"), float("nan")
    ok = dict(cols=32000, rows=1, inv_t=1.0, k=50, p=0.9)
    bad = [dict(cols=0), dict(cols=-3), dict(cols=65537), dict(rows=-1), dict(inv_t=0.0), dict(inv_t=-1.0), dict(inv_t=inf), dict(inv_t=nan),
           dict(p=-0.1), dict(p=1.5), dict(p=nan), dict(p=inf), dict(k=-1)]
    for change in bad:
        a = dict(ok, **change)
        # (null operands: a call that got past the checks to a launch would fault, not return)
        assert f(None, a["cols"], a["rows"], a["cols"], a["inv_t"], a["k"], a["p"], None, None, None, None, None) == -1, change
        assert NAME in L.last_error(), change
    for k, p in ((50, 0.9), (0, 1.0)):                            # the operands are checked next, filters on or off
        assert f(None, 32000, 1, 32000, 1.0, k, p, None, None, None, None, None) == -5
        assert NAME in L.last_error() and "null operand" in L.last_error()
    one = ctypes.c_void_p(16)                                     # (never dereferenced: the ld rule refuses first)
    assert f(one, 100, 2, 32000, 1.0, 50, 0.9, one, one, None, None, None) == -1 and NAME in L.last_error() and "ld=" in L.last_error()
    assert f(None, 32000, 0, 32000, 1.0, 50, 0.9, None, None, None, None, None) == 0             # no rows: nothing to do


def test_sample_rows_filtered_refuses_cpu_tensors():
    from medplib_amd import ops
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.sample_rows_filtered(torch.zeros(1, 8), torch.zeros(1), 1.0, top_k=2, top_p=0.9)


def test_worker_and_vqa_walk_parse_their_flags():
    from model.eval import vqa_infer as V
    from model.serve import model_worker as MW
    names = [n for n, _, _ in MW.FLAG_TABLE]
    assert len(names) == len(set(names)) and "apply-top-p" in names
    base = ["--model-path", "checkpoints/xxx", "--device_map", "cuda"]
    assert MW.parse_args(base).apply_top_p is False
    assert MW.parse_args(base + ["--apply-top-p"]).apply_top_p is True
    v = V.parse_args(["--version", "/ckpt", "--eval_vqa", "--temperature", "0.2", "--top_p", "0.9", "--num_beams", "1"])
    assert v.eval_vqa and v.temperature == 0.2 and v.top_p == 0.9 and v.num_beams == 1
    assert V.parse_args(["--version", "/ckpt"]).top_p is None and V.parse_args(["--version", "/ckpt"]).temperature == 0.0


def test_float64_rule_keeps_what_the_hf_warper_chain_keeps():
    """On float64 rows without ties (HF's sort splits a group of equal logits arbitrarily; the rule keeps or drops it whole) the kept set of
    kept_rule equals the finite entries HF's chain leaves, with HF's own switches: no TopK warper for k = 0, no TopP warper for p = 1."""
    try:
        from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    except Exception as e:                                         # noqa: BLE001
        pytest.skip(f"transformers' warpers do not import: {e}")
    g = torch.Generator().manual_seed(21)
    n = 0
    for cols in (63, 1000, 32011):
        for std in (0.5, 2.0, 8.0):
            row = torch.randn(cols, generator=g, dtype=torch.float64) * std
            for T in (0.2, 0.7, 1.0):
                for k in (0, 1, 5, 50):
                    for p in (0.1, 0.5, 0.9, 0.99, 1.0):
                        s = TemperatureLogitsWarper(T)(None, row.view(1, cols).clone())
                        if 0 < k:
                            s = TopKLogitsWarper(top_k=k)(None, s)
                        if p < 1.0:
                            s = TopPLogitsWarper(top_p=p)(None, s)
                        kept, _, _ = kept_rule(row.numpy(), T, k, p)
                        assert np.array_equal(kept, torch.isfinite(s[0]).numpy()), (cols, std, T, k, p, int(kept.sum()))
                        n += 1
    assert n == 3 * 3 * 3 * 4 * 5
