"""CPU: retrieval of in-context examples (model/rag/image_rag.py over medplib_amd/rag.py) without a GPU: the import face, the command line
and the record helpers against the executed reference (tests/golden/rag_reference.json), the new C-ABI entry points and their
refusals, and Pillow's bicubic coefficients (host C in the library) applied by a numpy restatement of the 8-bit pass against
PIL.Image.resize itself."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rag_cases  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "rag_reference.json")
NEW = ("mp_pil_resample_ksize", "mp_pil_resample_coeffs", "mp_image_table_crop_chw", "mp_dot_topk_workspace_bytes", "mp_dot_topk_f32",
       "mp_clip_pool_normalize_bf16", "mp_l2_normalize_rows_f32")


@pytest.fixture(scope="module")
def doc():
    return json.load(open(GOLD))


def test_import_face_resolves():
    from model.rag import image_rag as R
    from medplib_amd import rag
    for name in ("RAG_ENCODER_DEFAULT_PATHS", "resolve_path", "load_rgb", "normalize_features", "extract_target_mask",
                 "extract_query_image", "collect_candidates", "ImageRAGEncoder", "build_index", "load_index", "retrieve", "augment",
                 "parse_args"):
        assert hasattr(R, name), name
    assert R.ImageRAGEncoder is rag.ImageRAGEncoder and callable(R.ImageRAGEncoder.encode_paths)
    assert set(R.RAG_ENCODER_DEFAULT_PATHS) == {"clip_encoder", "med_encoder", "det_encoder", "mask_encoder"}


def _flag_table(parser):
    import argparse
    sub = next(a for a in parser._actions if isinstance(a, argparse._SubParsersAction))
    return {name: [[a.dest, list(a.option_strings), a.default, getattr(a.type, "__name__", None), a.choices, a.required]
                   for a in p._actions if a.dest != "help"] for name, p in sub.choices.items()}


def test_flag_table_equals_reference(doc):
    from model.rag import image_rag as R
    assert json.loads(json.dumps(_flag_table(R.build_parser()))) == doc["flags"]
    a = R.parse_args(["augment"])
    assert (a.command, a.top_k, a.batch_size, a.precision, a.device, a.rag_encoder_path) == ("augment", 3, 16, "bf16", "cuda", None)
    with pytest.raises(SystemExit):
        R.parse_args([])


def test_record_helpers_equal_reference(doc):
    from model.rag import image_rag as R
    recs = rag_cases.helper_records()
    assert json.loads(json.dumps(recs)) == doc["helper_records"]
    for r, want in zip(recs, doc["helpers"]):
        assert R.extract_query_image(r) == want["query_image"], r
        assert R.extract_target_mask(r) == want["target_mask"], r
        assert R.collect_candidates([r]) == want["candidates"], r
    assert R.collect_candidates(recs) == doc["all_candidates"]
    assert json.dumps(R.collect_candidates(rag_cases.candidate_records()), indent=2) == doc["metadata_json"]
    x = np.array(doc["normalize_features"]["in"], np.float32)
    got = R.normalize_features(x)
    assert got.dtype == np.float32 and np.array_equal(got, np.array(doc["normalize_features"]["out"], np.float32))


def test_resolve_path_and_load_rgb(tmp_path):
    from model.rag import image_rag as R
    rag_cases.write_images(str(tmp_path))
    assert R.resolve_path(None, "f") is None
    assert R.resolve_path(str(tmp_path / "vga.png"), "elsewhere") == str(tmp_path / "vga.png")
    assert R.resolve_path("vga.png", str(tmp_path)) == os.path.join(str(tmp_path), "vga.png")
    for name, (w, h, _) in rag_cases.IMAGES.items():
        a = R.load_rgb(str(tmp_path / name))
        assert a.dtype == np.uint8 and a.shape == (h, w, 3)
    with pytest.raises(FileNotFoundError, match="Cannot read image"):
        R.load_rgb(str(tmp_path / "missing.png"))
    (tmp_path / "bad.png").write_bytes(b"not an image")
    with pytest.raises(FileNotFoundError):
        R.load_rgb(str(tmp_path / "bad.png"))


def test_refusals_without_gpu_work(tmp_path):
    from medplib_amd import rag
    from medplib_amd.model.clip import vision_config_from_dir
    with pytest.raises(ValueError, match="Unsupported RAG encoder type"):
        rag.ImageRAGEncoder("text_encoder", str(tmp_path))
    for kw in (dict(precision="fp32"), dict(precision="fp16"), dict(device="cpu")):
        with pytest.raises(NotImplementedError, match="bf16 on the GPU"):
            rag.ImageRAGEncoder("clip_encoder", str(tmp_path), **kw)
    base = dict(model_type="clip_vision_model", hidden_size=1024, intermediate_size=4096, num_attention_heads=16, num_hidden_layers=24,
                image_size=336, patch_size=14, hidden_act="quick_gelu")
    json.dump(base, open(tmp_path / "config.json", "w"))
    cfg = vision_config_from_dir(str(tmp_path))
    assert (cfg.clip_hidden_size, cfg.clip_num_layers, cfg.clip_num_patches) == (1024, 24, 576)
    for field, bad in (("num_attention_heads", 8), ("hidden_act", "gelu"), ("intermediate_size", 4000), ("model_type", "siglip_vision_model")):
        json.dump(dict(base, **{field: bad}), open(tmp_path / "config.json", "w"))
        with pytest.raises(ValueError, match=field):
            vision_config_from_dir(str(tmp_path))
    json.dump({"resample": 2, "size": 336, "crop_size": 336}, open(tmp_path / "preprocessor_config.json", "w"))
    with pytest.raises(NotImplementedError, match="resample"):
        rag.processor_settings(str(tmp_path))
    json.dump({"size": 336, "crop_size": 336, "image_mean": [0.5] * 3, "image_std": [0.25] * 3}, open(tmp_path / "preprocessor_config.json", "w"))
    st = rag.processor_settings(str(tmp_path))
    assert st["shortest_edge"] == 336 and st["crop"] == (336, 336) and st["mean"] == (0.5, 0.5, 0.5)


def test_header_declares_and_library_exports_the_rag_entry_points():
    from medplib_amd import _lib
    protos = _lib.parse_header()
    assert all(n in protos for n in NEW), [n for n in NEW if n not in protos]
    if not os.path.exists(_lib.LIB_PATH):
        from medplib_amd import build
        build.build(verbose=False)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(dll, n) for n in NEW)


def test_dot_topk_refuses_bad_shapes():
    from medplib_amd import _lib
    L = _lib.lib()
    f = L.raw("mp_dot_topk_f32")
    for N, C, k, msg in ((100, 64, 0, "k must be in [1, 64]"), (100, 64, 65, "k must be in [1, 64]"), (100, 6, 3, "multiple of 4"),
                         (0, 64, 3, "N must be"), (1 << 31, 64, 3, "N must be")):
        assert f(None, C, None, N, 4, C, k, None, None, None, 0, None) == -1, (N, C, k)
        assert "mp_dot_topk_f32" in L.last_error() and msg in L.last_error(), L.last_error()
        assert L.raw("mp_dot_topk_workspace_bytes")(N, 4, C, k) == -1
    assert f(None, 60, None, 100, 4, 64, 3, None, None, None, 0, None) == -1 and "ld_index" in L.last_error()
    assert f(None, 64, None, 100, 4, 64, 3, None, None, None, 0, None) == -5 and "null operand" in L.last_error()
    assert L.raw("mp_dot_topk_workspace_bytes")(1 << 20, 1, 1024, 3) > 0
    assert L.raw("mp_clip_pool_normalize_bf16")(None, 2, 1, 64, None, None) == -1
    assert L.raw("mp_l2_normalize_rows_f32")(None, None, 0, 64, None) == -1
    assert L.raw("mp_image_table_crop_chw")(None, 300, 400, 3, None, None, 336, 336, 0, 0, 1, None) == -1
    assert L.raw("mp_pil_resample_ksize")(1, 100, 50) == 0
    b = np.zeros((50, 2), np.int32)
    assert L.raw("mp_pil_resample_coeffs")(4, 100, 50, b.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p), 5) == -5


def _apply_axis(a, bounds, coefs, axis):
    """Pillow's 8bpc pass restated: acc = 2^21 + sum(pixel * coeff) in int; clip8(acc >> 22)."""
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((bounds.shape[0],) + a.shape[1:], np.int64)
    for xx, (xmin, n) in enumerate(bounds):
        acc = np.full(a.shape[1:], 1 << 21, np.int64)
        for x in range(n):
            acc += a[xmin + x] * int(coefs[xx, x])
        out[xx] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out.astype(np.uint8), 0, axis)


def test_bicubic_coeffs_bit_equal_to_pil():
    from PIL import Image
    from medplib_amd.preprocess import PIL_BICUBIC, resample_coeffs_host
    rng = np.random.default_rng(5)
    sizes = [(40, 336), (336, 40), (1500, 336), (336, 1500), (2000, 336), (17, 336), (336, 336), (97, 411)]
    sizes += [tuple(int(v) for v in rng.integers(5, 1200, 2)) for _ in range(42)]
    for in_w, out_w in sizes:
        h = 3
        img = rng.integers(0, 256, (h, in_w, 3), dtype=np.uint8)
        ref = np.array(Image.fromarray(img).resize((out_w, h), Image.BICUBIC))
        b, c = resample_coeffs_host(PIL_BICUBIC, in_w, out_w)
        assert c.shape[1] == int(np.ceil(2 * max(in_w / out_w, 1.0))) * 2 + 1
        got = _apply_axis(img, b, c, 1) if in_w != out_w else img
        assert np.array_equal(got, ref), (in_w, out_w)
    img = rng.integers(0, 256, (413, 287, 3), dtype=np.uint8)       # both passes, horizontal first (as Pillow)
    ref = np.array(Image.fromarray(img).resize((336, 483), Image.BICUBIC))
    bw, cw = resample_coeffs_host(PIL_BICUBIC, 287, 336)
    bh, ch = resample_coeffs_host(PIL_BICUBIC, 413, 483)
    assert np.array_equal(_apply_axis(_apply_axis(img, bw, cw, 1), bh, ch, 0), ref)
