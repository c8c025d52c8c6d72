"""Command line and import face of the retrieval of in-context examples, at the reference's path and names (model/rag/image_rag.py, run
by scripts/build_medplib_icl_rag_index.sh and scripts/infer_medplib_icl_rag.sh):

    python model/rag/image_rag.py build   --candidate_json TRAIN.json --index_dir DIR [--image_folder F --batch_size 16 ...]
    python model/rag/image_rag.py augment --query_json TEST.json --output_json OUT.json --index_dir DIR [--top_k 3 ...]

`build` writes DIR/embeddings.npy (float32 [N, C]) and DIR/metadata.json; `augment` writes the query records with `image`,
`target_mask` and `icl_examples` set.  The work is done by medplib_amd/rag.py on the GPU (bf16 tower, exact fp32 search); the
flags are the reference's, and `--precision fp32/fp16` or `--device cpu` are refused with NotImplementedError."""
import argparse
import sys
from pathlib import Path

ROOT = str(Path(__file__).resolve().parents[2])
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from medplib_amd.rag import (RAG_ENCODER_DEFAULT_PATHS, ImageRAGEncoder, augment, build_index, collect_candidates,  # noqa: E402,F401
                             extract_query_image, extract_target_mask, load_index, load_rgb, normalize_features, resolve_path,
                             retrieve)


def build_parser():
    """The reference's command line: subcommands build / augment, the same flags, defaults and choices."""
    parser = argparse.ArgumentParser(description="Decoupled image-RAG for MedPLIB-ICL.")
    sub = parser.add_subparsers(dest="command", required=True)
    common = (("--rag_encoder_type", dict(default="clip_encoder", choices=list(RAG_ENCODER_DEFAULT_PATHS))),
              ("--rag_encoder_path", dict(default=None)),
              ("--image_folder", dict(default="/data/3/MedPLIB/dataset/images-and-masks-root")),
              ("--index_dir", dict(default="/data/3/MedPLIB/dataset/rag_index")),
              ("--batch_size", dict(type=int, default=16)),
              ("--device", dict(default="cuda")),
              ("--precision", dict(choices=["fp32", "bf16", "fp16"], default="bf16")))
    own = {"build": (("--candidate_json", dict(default="/data/3/MedPLIB/dataset/MedPLIB_ICL_train.json")),),
           "augment": (("--query_json", dict(default="/data/3/MedPLIB/dataset/MedPLIB_ICL_test.json")),
                       ("--output_json", dict(default="/data/3/MedPLIB/dataset/MedPLIB_ICL_RAG_test.json")),
                       ("--top_k", dict(type=int, default=3)))}
    for name, extra in own.items():
        p = sub.add_parser(name)
        for flag, kw in common + extra:
            p.add_argument(flag, **kw)
    return parser


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    {"build": build_index, "augment": augment}[args.command](args)


if __name__ == "__main__":
    main()
