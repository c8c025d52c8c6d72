"""Writes tests/golden/rag_reference.{npz,json} by EXECUTING the reference's model/rag/image_rag.py (development container only: it
needs the reference tree and transformers; it never runs on the GPU machine and is not part of oracle/).

    python scripts/make_rag_golden.py /path/to/reference

The reference reads images with cv2, which is not installed: a stub built on PIL stands in (`imread` -> BGR uint8 of
Image.convert("RGB"), None when unreadable; `cvtColor` flips the channels).  Without a GPU the reference runs CPU fp32: the installed
transformers' PIL-backend CLIPImageProcessor and an fp32 CLIPVisionModel.  The checkpoint is a tiny random CLIPVisionModel (hidden 128,
2 heads, intermediate 256, 2 layers, image 336, patch 14) with the CLIP-L-336 preprocessor_config.json.  Its weights are int8 codes x
2^e per tensor (exact in fp32 and bf16), stored lzma-compressed with their shapes and exponents so the tests can write the checkpoint
back out exactly.  The processor's pixel values are stored losslessly as per-channel value tables + row-delta uint8 codes
(tests/rag_cases.pack_pixel_values), also lzma-compressed."""
import argparse
import importlib.util
import io
import json
import os
import sys
import tempfile
import types
from contextlib import redirect_stdout

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rag_cases  # noqa: E402

PREPROCESSOR_CONFIG = {                     # openai/clip-vit-large-patch14-336
    "crop_size": 336, "do_center_crop": True, "do_normalize": True, "do_resize": True,
    "feature_extractor_type": "CLIPFeatureExtractor", "image_mean": [0.48145466, 0.4578275, 0.40821073],
    "image_std": [0.26862954, 0.26130258, 0.27577711], "resample": 3, "size": 336}
TINY = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=336, patch_size=14,
            projection_dim=64, hidden_act="quick_gelu", layer_norm_eps=1e-5)


def cv2_stub():
    from PIL import Image
    m = types.ModuleType("cv2")
    m.COLOR_BGR2RGB = 4

    def imread(path):
        try:
            return np.ascontiguousarray(np.array(Image.open(path).convert("RGB"))[:, :, ::-1])
        except Exception:
            return None
    m.imread = imread
    m.cvtColor = lambda img, code: np.ascontiguousarray(img[:, :, ::-1])
    return m


def write_checkpoint(path, seed=5):
    from transformers import CLIPVisionConfig, CLIPVisionModel
    torch.manual_seed(seed)
    model = CLIPVisionModel(CLIPVisionConfig(**TINY)).eval()
    with torch.no_grad():                   # spread the LayerNorm affine and biases away from their 1 / 0 init
        for n, p in model.named_parameters():
            if "norm" in n and n.endswith("weight"):
                p.add_(torch.randn_like(p) * 0.1)
            elif n.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.05)
        packed = {}
        for n, p in model.named_parameters():     # int8 codes x 2^e per tensor: exact in fp32 and bf16, and small to store
            e = int(np.ceil(np.log2(float(p.abs().max()) / 127)))
            codes = torch.round(torch.ldexp(p, torch.tensor(-e))).clamp(-127, 127)
            p.copy_(torch.ldexp(codes, torch.tensor(e)))
            packed[n] = (codes.to(torch.int8).numpy(), e)
    model.save_pretrained(path)
    json.dump(PREPROCESSOR_CONFIG, open(os.path.join(path, "preprocessor_config.json"), "w"), indent=2)
    assert set(packed) == set(model.state_dict())
    return packed


def flag_table(parser):
    """{subcommand: [[dest, option strings, default, type name, choices, required], ...]} of an argparse parser with subcommands."""
    out = {}
    sub = next(a for a in parser._actions if isinstance(a, argparse._SubParsersAction))
    for name, p in sub.choices.items():
        out[name] = [[a.dest, list(a.option_strings), a.default, getattr(a.type, "__name__", None), a.choices, a.required]
                     for a in p._actions if a.dest != "help"]
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit("usage: python scripts/make_rag_golden.py /path/to/reference")
    ref = sys.argv[1]
    sys.modules["cv2"] = cv2_stub()
    spec = importlib.util.spec_from_file_location("ref_image_rag", os.path.join(ref, "model", "rag", "image_rag.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    work = tempfile.mkdtemp()
    ckpt, imgs, idx = (os.path.join(work, d) for d in ("ckpt", "images", "index"))
    weights = write_checkpoint(ckpt)
    rag_cases.write_images(imgs)
    json.dump(rag_cases.candidate_records(), open(os.path.join(work, "cand.json"), "w"))
    json.dump(rag_cases.query_records(), open(os.path.join(work, "query.json"), "w"))

    enc = R.ImageRAGEncoder("clip_encoder", ckpt, device="cuda", precision="bf16")
    assert enc.device == "cpu"
    names = sorted(rag_cases.IMAGES)
    pixel_values = np.stack([enc.processor(images=[R.load_rgb(os.path.join(imgs, n))], return_tensors="pt")["pixel_values"][0].numpy()
                             for n in names])
    emb_images = enc.encode_paths([os.path.join(imgs, n) for n in names], batch_size=3)

    common = dict(rag_encoder_type="clip_encoder", rag_encoder_path=ckpt, image_folder=imgs, index_dir=idx, batch_size=16,
                  device="cuda", precision="bf16")
    out = io.StringIO()
    with redirect_stdout(out):
        R.build_index(argparse.Namespace(candidate_json=os.path.join(work, "cand.json"), **common))
    build_line = out.getvalue().replace(idx, "<index_dir>").strip()
    embeddings = np.load(os.path.join(idx, "embeddings.npy"))
    metadata_text = open(os.path.join(idx, "metadata.json")).read()
    loaded, _ = R.load_index(idx)
    qpaths = [R.resolve_path(R.extract_query_image(it), imgs) for it in rag_cases.query_records()]
    qfeat = enc.encode_paths(qpaths, batch_size=16)
    scores = np.stack([loaded @ q for q in qfeat])
    aug_path = os.path.join(work, "out", "aug.json")
    with redirect_stdout(io.StringIO()):
        R.augment(argparse.Namespace(query_json=os.path.join(work, "query.json"), output_json=aug_path, top_k=3, **common))

    parser = {}
    orig = argparse.ArgumentParser.parse_args

    def capture(self, *a, **k):
        parser.setdefault("p", self)
        return orig(self, ["build"])
    argparse.ArgumentParser.parse_args = capture
    try:
        R.parse_args()
    finally:
        argparse.ArgumentParser.parse_args = orig

    helpers = [{"query_image": R.extract_query_image(r), "target_mask": R.extract_target_mask(r), "candidates": R.collect_candidates([r])}
               for r in rag_cases.helper_records()]
    gold = os.path.join(ROOT, "tests", "golden")
    table, delta = rag_cases.pack_pixel_values(pixel_values.astype(np.float32))
    assert np.array_equal(rag_cases.unpack_pixel_values(table, delta).view(np.uint32), pixel_values.astype(np.float32).view(np.uint32))
    wnames = sorted(weights)
    wflat = np.concatenate([weights[k][0].ravel() for k in wnames]).view(np.uint8)
    doc_weights = [[k, list(weights[k][0].shape), weights[k][1]] for k in wnames]
    np.savez_compressed(os.path.join(gold, "rag_reference.npz"), pixel_table=table,
                        pixel_codes_delta=rag_cases.pack_bytes(delta), weight_codes=rag_cases.pack_bytes(wflat),
                        embeddings_images=emb_images.astype(np.float32), embeddings=embeddings, index_loaded=loaded,
                        query_features=qfeat.astype(np.float32), scores=scores.astype(np.float32))
    doc = {"image_names": names, "pixel_values_shape": list(pixel_values.shape), "weights": doc_weights, "tiny_config": TINY, "preprocessor_config": PREPROCESSOR_CONFIG,
           "candidate_records": rag_cases.candidate_records(), "query_records": rag_cases.query_records(),
           "helper_records": rag_cases.helper_records(), "helpers": helpers,
           "all_candidates": R.collect_candidates(rag_cases.helper_records()), "metadata_json": metadata_text,
           "augmented_json": open(aug_path).read(), "build_line": build_line, "flags": flag_table(parser["p"]),
           "normalize_features": {"in": [[3.0, 4.0], [0.0, 0.0], [1e-7, -2e-7]],
                                  "out": R.normalize_features(np.array([[3.0, 4.0], [0.0, 0.0], [1e-7, -2e-7]], np.float32)).tolist()}}
    json.dump(doc, open(os.path.join(gold, "rag_reference.json"), "w"), indent=1)
    print("wrote", gold, "rag_reference.{npz,json};", build_line)


if __name__ == "__main__":
    main()
