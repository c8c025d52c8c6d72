"""Retrieval of in-context examples: the image RAG of the ICL workflow (model/rag/image_rag.py, scripts/build_medplib_icl_rag_index.sh,
scripts/infer_medplib_icl_rag.sh), written for this build.

`build` embeds every (image, mask) candidate of an ICL training JSON with a CLIP vision tower and stores the rows; `augment` embeds every
query image and gives each query its `top_k` most similar candidates as `icl_examples`.  The embedding is the L2-normalised bf16 mean
of the tower's last hidden state over the patch rows; the similarity is the inner product of the normalised rows.

Device work: decoding runs on a pool of at most 16 host threads while the device preprocesses (`preprocess_clip_processor`, the
CLIPImageProcessor bit for bit), runs the full-depth tower (`ClipTower.encode_pooled`) and ranks (`ops.dot_topk`, exact fp32; one batched
call for all queries).  Only bf16 on the GPU is built: there is no CPU path."""
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import ops
from . import preprocess as P

RAG_ENCODER_DEFAULT_PATHS = {
    "clip_encoder": "/data/3/MedPLIB/checkpoint/clip-vit-large-patch14-336",
    "med_encoder": "/data/3/MedPLIB/checkpoint/med_encoder",
    "det_encoder": "/data/3/MedPLIB/checkpoint/det_encoder",
    "mask_encoder": "/data/3/MedPLIB/checkpoint/mask_encoder",
}

MAX_DECODE_WORKERS = 16
TOPK_WORKSPACE_BUDGET = 256 << 20          # bytes of partial lists per dot_topk call; augment splits its queries beyond this


# ------------------------------------------------------------------ record helpers
def resolve_path(path, image_folder):
    """An existing path as given; anything else is taken relative to `image_folder` (None stays None)."""
    if path is None or os.path.exists(path):
        return path
    return os.path.join(image_folder, path)


def load_rgb(path):
    """uint8 [H, W, 3] RGB of an image file; FileNotFoundError when it cannot be read."""
    from .dataset import _open_rgb
    try:
        return _open_rgb(path)
    except (OSError, ValueError, TypeError, AttributeError):
        raise FileNotFoundError(f"Cannot read image: {path}") from None


def normalize_features(features):
    """Rows divided by their L2 norm + 1e-12, in the array's own precision (host helper; the search path uses ops.l2_normalize_rows)."""
    denom = np.linalg.norm(features, axis=-1, keepdims=True)
    denom = denom + 1e-12
    return features / denom


def _numbered(item, stem):
    """Sorted N of the keys `<stem>N` of a record (the key with every `stem` removed must be all digits)."""
    return sorted(int(key.replace(stem, "")) for key in item if key.startswith(stem) and key.replace(stem, "").isdigit())


def extract_target_mask(item):
    """The query's mask: `target_mask`, `mask` or `mask3` (first one set), else the text between the first <mask> and </mask> of a
    conversation turn, else None."""
    found = next((item[key] for key in ("target_mask", "mask", "mask3") if item.get(key) is not None), None)
    if found is not None:
        return found
    for turn in item.get("conversations", []):
        text = str(turn.get("value", ""))
        lo, hi = text.find("<mask>"), text.find("</mask>")
        if lo >= 0 and hi > lo:
            return text[lo + 6:hi]
    return None


def extract_query_image(item):
    """`image` when set, else the highest-numbered `imageN`, else None."""
    if item.get("image") is not None:
        return item["image"]
    nums = _numbered(item, "image")
    return item[f"image{nums[-1]}"] if nums else None


def collect_candidates(items):
    """Every (image, mask) pair of the records, in record order: the query pair, then the `icl_examples` (or `examples`) pairs, then the
    `imageN` / `maskN` pairs in N order.  Repeated pairs are kept."""
    out = []

    def take(image, mask):
        if image is not None and mask is not None:
            out.append({"image": image, "mask": mask})
    for item in items:
        take(extract_query_image(item), extract_target_mask(item))
        for ex in item.get("icl_examples", item.get("examples", [])):
            take(ex.get("image"), ex.get("mask"))
        for n in _numbered(item, "image"):
            take(item.get(f"image{n}"), item.get(f"mask{n}"))
    return out


# ------------------------------------------------------------------ processor config
def processor_settings(path):
    """preprocessor_config.json of a CLIP checkpoint -> the arguments of preprocess_clip_processor.  Settings the device path does
    not build raise NotImplementedError naming the field."""
    f = os.path.join(path, "preprocessor_config.json")
    cfg = json.load(open(f)) if os.path.exists(f) else {}
    for key, want in (("do_resize", True), ("do_center_crop", True), ("do_rescale", True), ("do_normalize", True)):
        if cfg.get(key, want) is not want:
            raise NotImplementedError(f"{f}: {key}={cfg.get(key)!r} is not built (the device path always does it)")
    size = cfg.get("size", {"shortest_edge": 224})
    if isinstance(size, dict):
        if "shortest_edge" not in size:
            raise NotImplementedError(f"{f}: size={size!r} is not built (only {{'shortest_edge': s}})")
        size = size["shortest_edge"]
    crop = cfg.get("crop_size", {"height": 224, "width": 224})
    crop = (crop["height"], crop["width"]) if isinstance(crop, dict) else (int(crop), int(crop))
    resample = int(cfg.get("resample", P.PIL_BICUBIC))
    if resample != P.PIL_BICUBIC:
        raise NotImplementedError(f"{f}: resample={resample} is not built (only 3, PIL BICUBIC)")
    return dict(shortest_edge=int(size), crop=crop, mean=tuple(cfg.get("image_mean", P.CLIP_MEAN)),
                std=tuple(cfg.get("image_std", P.CLIP_STD)), rescale_factor=float(cfg.get("rescale_factor", 1 / 255)))


# ------------------------------------------------------------------ encoder
class ImageRAGEncoder:
    """CLIP image embeddings on the GPU: decode on host threads, CLIPImageProcessor + full-depth bf16 tower + pooling on the device."""

    def __init__(self, encoder_type="clip_encoder", encoder_path=None, device="cuda", precision="bf16"):
        if encoder_type not in RAG_ENCODER_DEFAULT_PATHS:
            raise ValueError(f"Unsupported RAG encoder type: {encoder_type}. Choose from {list(RAG_ENCODER_DEFAULT_PATHS.keys())}.")
        if precision != "bf16":
            raise NotImplementedError(f"precision={precision!r}: this build runs the CLIP tower in bf16 on the GPU only")
        if str(device).startswith("cpu") or not torch.cuda.is_available():
            raise NotImplementedError(f"device={device!r}: this build runs the CLIP tower in bf16 on the GPU only (no CPU path)")
        from .model.clip import ClipTower
        self.encoder_type = encoder_type
        self.encoder_path = encoder_path or RAG_ENCODER_DEFAULT_PATHS[encoder_type]
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.settings = processor_settings(self.encoder_path)
        with torch.cuda.device(self.device):
            self.tower = ClipTower.from_vision_dir(self.encoder_path, self.device)
        size = self.tower.cfg.clip_image_size
        if self.settings["crop"] != (size, size):
            raise ValueError(f"{self.encoder_path}: crop_size {self.settings['crop']} != the tower's image_size {size}")

    def _pixels(self, rgb):
        img = torch.from_numpy(np.ascontiguousarray(rgb)).to(self.device, non_blocking=True)
        return P.preprocess_clip_processor(img, out_dtype=torch.bfloat16, **self.settings)

    @torch.no_grad()
    def encode_paths_device(self, paths, batch_size=16):
        """-> [len(paths), C] f32 on the device, L2-normalised rows.  Images are decoded up to one batch ahead on the host pool."""
        if batch_size < 1:
            raise ValueError(f"batch_size must be >= 1, got {batch_size}")
        out = []
        with torch.cuda.device(self.device), ThreadPoolExecutor(max_workers=min(MAX_DECODE_WORKERS, max(1, batch_size))) as pool:
            futs = [pool.submit(load_rgb, p) for p in paths[:2 * batch_size]]
            nxt = len(futs)
            for start in range(0, len(paths), batch_size):
                stop = min(start + batch_size, len(paths))
                pix = torch.stack([self._pixels(futs[i].result()) for i in range(start, stop)])
                for i in range(start, stop):
                    futs[i] = None
                futs += [pool.submit(load_rgb, p) for p in paths[nxt:stop + 2 * batch_size]]
                nxt = len(futs)
                out.append(self.tower.encode_pooled(pix))
        if not out:
            return torch.empty((0, self.tower.cfg.clip_hidden_size), dtype=torch.float32, device=self.device)
        return torch.cat(out)

    def encode_paths(self, paths, batch_size=16):
        """-> numpy [len(paths), C] float32, L2-normalised rows."""
        return self.encode_paths_device(paths, batch_size).cpu().numpy()


# ------------------------------------------------------------------ index and search
def _index_on_device(embeddings, device):
    x = torch.from_numpy(np.ascontiguousarray(embeddings, dtype=np.float32)).to(device)
    return ops.l2_normalize_rows(x, out=x)


def build_index(args):
    items = json.load(open(args.candidate_json, "r"))
    candidates = collect_candidates(items)
    if not candidates:
        raise ValueError("No image/mask candidates found.")
    encoder = ImageRAGEncoder(args.rag_encoder_type, args.rag_encoder_path, args.device, args.precision)
    emb = encoder.encode_paths([resolve_path(c["image"], args.image_folder) for c in candidates], batch_size=args.batch_size)
    os.makedirs(args.index_dir, exist_ok=True)
    np.save(os.path.join(args.index_dir, "embeddings.npy"), emb)
    with open(os.path.join(args.index_dir, "metadata.json"), "w") as f:
        json.dump(candidates, f, indent=2)
    print(f"Saved {len(candidates)} candidates to {args.index_dir}")


def load_index(index_dir, device="cuda"):
    """(rows normalised once more, as numpy float32, metadata list).  The normalisation runs on the device."""
    emb = np.load(os.path.join(index_dir, "embeddings.npy"))
    with open(os.path.join(index_dir, "metadata.json"), "r") as f:
        metadata = json.load(f)
    return _index_on_device(emb, device).cpu().numpy(), metadata


def _check_k(top_k):
    if top_k < 0 or top_k > ops.TOPK_MAX:
        raise ValueError(f"top_k={top_k}: the search returns 0 <= top_k <= {ops.TOPK_MAX} examples")


def retrieve(query_feature, embeddings, metadata, top_k, device="cuda"):
    """The `top_k` entries of `metadata` whose rows have the largest inner product with `query_feature` (fewer when the index is
    smaller), best first, ties to the lower row (one Q = 1 dot_topk)."""
    _check_k(top_k)
    if top_k == 0:
        return []
    index = torch.from_numpy(np.ascontiguousarray(embeddings, dtype=np.float32)).to(device)
    q = torch.from_numpy(np.ascontiguousarray(query_feature, dtype=np.float32).reshape(1, -1)).to(device)
    _, idx = ops.dot_topk(index, q, top_k)
    return [metadata[i] for i in idx[0].cpu().tolist() if i >= 0]


def search(index, queries, top_k):
    """Device index [N, C] and queries [Q, C] -> int32 [Q, top_k] row ids (-1 past N), in as few dot_topk calls as the workspace budget
    allows (one for any realistic query set)."""
    N, C = index.shape
    Q = queries.shape[0]
    per_query = max(1, ops.dot_topk_workspace_bytes(N, Q, C, top_k) // max(Q, 1))
    step = max(1, min(Q, TOPK_WORKSPACE_BUDGET // per_query))
    return torch.cat([ops.dot_topk(index, queries[s:s + step], top_k)[1] for s in range(0, Q, step)])


def augment(args):
    items = json.load(open(args.query_json, "r"))
    _check_k(args.top_k)
    encoder = ImageRAGEncoder(args.rag_encoder_type, args.rag_encoder_path, args.device, args.precision)
    emb = np.load(os.path.join(args.index_dir, "embeddings.npy"))
    with open(os.path.join(args.index_dir, "metadata.json"), "r") as f:
        metadata = json.load(f)
    with torch.cuda.device(encoder.device):
        index = _index_on_device(emb, encoder.device)              # uploaded and normalised while the queries decode
        queries = encoder.encode_paths_device([resolve_path(extract_query_image(it), args.image_folder) for it in items],
                                              batch_size=args.batch_size)
        ids = search(index, queries, args.top_k).cpu().tolist() if args.top_k > 0 and items else [[] for _ in items]
    result = []
    for item, row in zip(items, ids):
        rec = dict(item)
        rec["image"] = extract_query_image(rec)
        mask = extract_target_mask(rec)
        if mask is not None:
            rec["target_mask"] = mask
        rec["icl_examples"] = [metadata[i] for i in row if i >= 0]
        result.append(rec)
    if os.path.dirname(args.output_json):
        os.makedirs(os.path.dirname(args.output_json), exist_ok=True)
    with open(args.output_json, "w") as f:
        json.dump(result, f, indent=2)
    print(f"Saved RAG-augmented ICL JSON to {args.output_json}")
