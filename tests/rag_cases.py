"""Shared inputs of the retrieval tests and of scripts/make_rag_golden.py: seeded PNG images of the shapes CLIPImageProcessor meets
(square at the crop size, landscape, portrait, upscaled from 224 and from 97 x 411, 640 x 480, grayscale, RGBA), the ICL records that
reference them, and crafted records for every branch of the record helpers."""
import os

import numpy as np

# name -> (width, height, PIL mode)
IMAGES = {
    "sq336.png": (336, 336, "RGB"),
    "land.png": (517, 389, "RGB"),
    "port.png": (301, 533, "RGB"),
    "up224.png": (224, 224, "RGB"),
    "up97x411.png": (97, 411, "RGB"),
    "vga.png": (640, 480, "RGB"),
    "gray.png": (402, 299, "L"),
    "rgba.png": (353, 421, "RGBA"),
}


def image_array(name):
    """Seeded smooth-plus-noise uint8 image of IMAGES[name] (H x W x channels of its mode).  The noise is mild so that the fixture's
    pixel values compress; the random-size sweep of the GPU test covers full-range noise."""
    w, h, mode = IMAGES[name]
    rng = np.random.default_rng(sorted(IMAGES).index(name) + 11)
    ch = {"RGB": 3, "L": 1, "RGBA": 4}[mode]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([128 + 100 * np.sin(xx / (7 + 5 * c + rng.uniform(0, 20)) + yy / (11 + rng.uniform(0, 30)) + rng.uniform(0, 6))
                     for c in range(ch)], -1)
    a = np.clip(base + rng.normal(0, 0.5, base.shape), 0, 255).astype(np.uint8)
    return a[:, :, 0] if ch == 1 else a


def write_images(folder):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for name, (_, _, mode) in IMAGES.items():
        Image.fromarray(image_array(name), mode=mode).save(os.path.join(folder, name))
    return folder


def candidate_records():
    """ICL training records: every candidate source of collect_candidates, and one image (vga.png) with two masks, which gives two
    exactly tied candidates."""
    return [
        {"image": "sq336.png", "mask": "m/sq.png", "conversations": [{"from": "human", "value": "<image> segment"}]},
        {"image": "land.png", "conversations": [{"from": "human", "value": "find <mask>m/land.png</mask> here"}],
         "icl_examples": [{"image": "port.png", "mask": "m/port.png"}, {"image": "up224.png"}]},
        {"image1": "up97x411.png", "mask1": "m/u97.png", "image2": "vga.png", "mask2": "m/vga_a.png",
         "conversations": [{"from": "gpt", "value": "ok"}]},
        {"image": "vga.png", "target_mask": "m/vga_b.png", "examples": [{"image": "gray.png", "mask": "m/gray.png"}]},
        {"image": "rgba.png", "mask3": "m/rgba.png"},
    ]


def query_records():
    """ICL test records for `augment` (the query image comes from `image` or the highest `imageN`)."""
    return [
        {"id": 0, "image": "land.png", "mask": "m/q0.png", "conversations": [{"from": "human", "value": "<image> q0"}]},
        {"id": 1, "image1": "gray.png", "image3": "vga.png", "conversations": [{"from": "human", "value": "x <mask>m/q1.png</mask>"}]},
        {"id": 2, "image": "up224.png"},
        {"id": 3, "image": "rgba.png", "target_mask": "m/q3.png"},
        {"id": 4, "image": "sq336.png"},
        {"id": 5, "image": "up97x411.png", "mask3": "m/q5.png"},
    ]


def helper_records():
    """Records for every branch of extract_target_mask / extract_query_image / collect_candidates."""
    return [
        {},
        {"image": None, "mask": None},
        {"image": "a.png", "target_mask": "t.png", "mask": "m.png"},
        {"image": "a.png", "target_mask": None, "mask": "m.png", "mask3": "m3.png"},
        {"image": "a.png", "mask3": "m3.png"},
        {"image": "a.png", "conversations": [{"value": "no tags"}, {"value": "x </mask> y <mask>late"},
                                             {"value": "p <mask>first.png</mask> q <mask>second.png</mask>"}]},
        {"image": "a.png", "conversations": [{"value": "<mask></mask>"}]},
        {"image": "a.png", "conversations": [{"from": "human"}, {"value": 12}]},
        {"image2": "b2.png", "image10": "b10.png", "image": None, "mask10": "k10.png", "mask2": "k2.png"},
        {"image7": "c7.png", "imageX": "cx.png", "image": None, "mask": "q.png", "mask7": None},
        {"image": "d.png", "mask": "dm.png", "icl_examples": [{"image": "e.png", "mask": "em.png"}, {"image": "f.png"}, {"mask": "g.png"}],
         "examples": [{"image": "never.png", "mask": "never.png"}]},
        {"image": "h.png", "examples": [{"image": "i.png", "mask": "im.png"}], "image1": "j.png", "mask1": "jm.png",
         "image3": "l.png", "mask3": "lm.png"},
        {"image": "a.png", "mask": "m.png", "icl_examples": []},
        {"image": "dup.png", "mask": "dm.png", "image1": "dup.png", "mask1": "dm.png"},
    ]


def pack_pixel_values(pv):
    """Lossless compact form of CLIPImageProcessor output [n, 3, H, W] f32: every channel holds at most 256 distinct values (one per
    input byte), so it is stored as a per-channel table of them [3, 256] (NaN-padded) and uint8 codes, row-delta coded (mod 256) so
    that the smooth images compress."""
    table = np.full((3, 256), np.nan, np.float32)
    codes = np.empty(pv.shape, np.uint8)
    for c in range(3):
        vals = np.unique(pv[:, c])
        assert len(vals) <= 256
        table[c, :len(vals)] = vals
        codes[:, c] = np.searchsorted(vals, pv[:, c])
    delta = codes.copy()
    delta[..., 1:] = codes[..., 1:] - codes[..., :-1]
    return table, delta


def unpack_pixel_values(table, delta):
    codes = np.cumsum(delta, axis=-1, dtype=np.uint8)
    return np.stack([table[c][codes[:, c]] for c in range(3)], 1)


def int8_weight(codes, exp):
    """Fixture checkpoint tensors are int8 codes x 2^exp (exact in bf16 and fp32) -> float32."""
    return np.ldexp(codes.astype(np.float32), int(exp))


def pack_bytes(a):
    """uint8 array -> lzma-compressed bytes (as a uint8 array, for an npz)."""
    import lzma
    return np.frombuffer(lzma.compress(np.ascontiguousarray(a).tobytes(), preset=9 | lzma.PRESET_EXTREME), np.uint8)


def unpack_bytes(packed, shape, dtype):
    import lzma
    return np.frombuffer(lzma.decompress(packed.tobytes()), dtype).reshape(shape)
