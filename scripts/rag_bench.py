"""Retrieval of in-context examples on one MI355X -> profiles/rag_bench.json (or the path given by --out).

  encode   images/s of preprocess (CLIPImageProcessor on the device) + full-depth CLIP-L-336 tower + pooling from pre-decoded uint8
           images already on the device, batch 16 and 64; fraction of the bf16 MFMA peak at 2 x 303 M MAC x 577 tokens per image.
  build    wall time of `build`'s encode over synthetic PNGs (decode on <= 16 host threads overlapping the device), with the host
           decode alone and the device work alone timed separately.
  search   dot_topk (exact fp32): Q = 1 over N = 1 048 576 x 1024 (4.3 GB, beyond the 256 MB Infinity Cache) as a fraction of 8 TB/s,
           Q = 1024 over N = 262 144 as a fraction of the 157.3 TF fp32 peak; torch.mm + torch.topk timed in the same process as a
           comparator only (it is not on any path)."""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16_PEAK, F32_PEAK, HBM = 2516.6e12, 157.3e12, 8.0e12


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps / 1e3


def tower_flop(cfg):
    C, I, S, p = cfg.clip_hidden_size, cfg.clip_intermediate_size, cfg.clip_num_patches + 1, cfg.clip_patch_size
    per_layer = 2 * S * (4 * C * C + 2 * C * I) + 2 * 2 * S * S * C
    return cfg.clip_num_layers * per_layer + 2 * cfg.clip_num_patches * 3 * p * p * C


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rag_bench.json"))
    ap.add_argument("--n_png", type=int, default=2000)
    args = ap.parse_args()
    from medplib_amd import ops
    from medplib_amd import preprocess as P
    from medplib_amd import rag
    from medplib_amd.model.clip import ClipTower
    from medplib_amd.model.config import MedPLIBConfig
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0)}

    cfg = MedPLIBConfig(hidden_size=64, intermediate_size=64, mm_vision_select_layer=-1)
    tower = ClipTower(cfg, dev)
    flop = tower_flop(cfg)
    res["tower_tflop_per_image"] = flop / 1e12
    st = dict(shortest_edge=336, crop=(336, 336), mean=P.CLIP_MEAN, std=P.CLIP_STD)
    rng = np.random.default_rng(0)
    shapes = [(480, 640), (512, 512), (600, 400), (336, 336)]
    for bs in (16, 64):
        imgs = [torch.from_numpy(rng.integers(0, 256, shapes[i % 4] + (3,), dtype=np.uint8)).to(dev) for i in range(bs)]

        def run():
            pix = torch.stack([P.preprocess_clip_processor(x, out_dtype=torch.bfloat16, **st) for x in imgs])
            return tower.encode_pooled(pix)
        t = timed(run, 5)
        res[f"encode_bs{bs}"] = {"s_per_batch": t, "images_per_s": bs / t, "bf16_peak_fraction": bs * flop / t / BF16_PEAK}
        print("encode", bs, res[f"encode_bs{bs}"], flush=True)

    # build: synthetic PNGs through the encoder's decode pool and device path
    from PIL import Image
    tmp = tempfile.mkdtemp()
    paths = []
    for i in range(args.n_png):
        h, w = shapes[i % 4]
        p = os.path.join(tmp, f"{i}.png")
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(p, compress_level=1)
        paths.append(p)
    enc = rag.ImageRAGEncoder.__new__(rag.ImageRAGEncoder)
    enc.device, enc.settings, enc.tower = dev, st, tower
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=rag.MAX_DECODE_WORKERS) as pool:
        decoded = list(pool.map(rag.load_rgb, paths))
    t_decode = time.perf_counter() - t0
    dev_imgs = [torch.from_numpy(x).to(dev) for x in decoded[:64]]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(0, args.n_png, 16):
        pix = torch.stack([P.preprocess_clip_processor(dev_imgs[(s + j) % 64], out_dtype=torch.bfloat16, **st) for j in range(16)])
        tower.encode_pooled(pix)
    torch.cuda.synchronize()
    t_device = time.perf_counter() - t0
    t0 = time.perf_counter()
    emb = enc.encode_paths_device(paths, batch_size=16)
    torch.cuda.synchronize()
    t_wall = time.perf_counter() - t0
    res["build_2000_png"] = {"n": args.n_png, "wall_s": t_wall, "host_decode_only_s": t_decode, "device_only_s": t_device,
                             "bound_by": "decode" if t_decode > t_device else "device", "rows": list(emb.shape)}
    print("build", res["build_2000_png"], flush=True)
    del decoded, dev_imgs

    # search
    g = torch.Generator(device=dev).manual_seed(0)
    C = 1024
    N = 1 << 20
    index = torch.randn(N, C, generator=g, device=dev)
    q = torch.randn(1, C, generator=g, device=dev)
    ws = torch.empty(max(8, ops.dot_topk_workspace_bytes(N, 1, C, 3)), dtype=torch.uint8, device=dev)
    t = timed(lambda: ops.dot_topk(index, q, 3, workspace=ws), 10)
    tt = timed(lambda: torch.topk(torch.mv(index, q[0]), 3), 10)
    res["search_q1_n1m"] = {"s": t, "TB_per_s": N * C * 4 / t / 1e12, "hbm_fraction": N * C * 4 / t / HBM, "torch_mv_topk_s": tt,
                            "speedup_vs_torch": tt / t}
    print("search q1", res["search_q1_n1m"], flush=True)
    del index
    N, Q = 262144, 1024
    index = torch.randn(N, C, generator=g, device=dev)
    qs = torch.randn(Q, C, generator=g, device=dev)
    ws = torch.empty(max(8, ops.dot_topk_workspace_bytes(N, Q, C, 3)), dtype=torch.uint8, device=dev)
    t = timed(lambda: ops.dot_topk(index, qs, 3, workspace=ws), 3)
    tt = timed(lambda: torch.topk(torch.mm(qs, index.T), 3, dim=1), 3)
    res["search_q1024_n262k"] = {"s": t, "TFLOPs": 2 * Q * N * C / t / 1e12, "f32_peak_fraction": 2 * Q * N * C / t / F32_PEAK,
                                 "torch_mm_topk_s": tt, "speedup_vs_torch": tt / t}
    print("search q1024", res["search_q1024_n262k"], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=2)


if __name__ == "__main__":
    main()
