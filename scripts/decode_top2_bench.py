"""Top-2 MoE decode rate at the 7B dimensions (32 decoder layers, every layer MoE): evaluate() at batch 1, ms per decode step as the slope
between two lengths (bench.py decode_rate's method: prefill and the one-off graph capture cancel, the fastest of three calls per length
after one untimed call), for
    top-1 E = 2, captured graph   (bench.py's decode object, for reference)
    top-2 E = 3, token-by-token loop   (how top-2 models decoded before the fused top-2 path)
    top-2 E = 3, captured graph
and the HBM fraction of the weights each step streams: attention + k experts' MLPs per layer + lm_head (k = 1 or 2).
python scripts/decode_top2_bench.py [--new 32] [--out FILE]"""
import argparse
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from medplib_amd.model.config import MedPLIBConfig
from medplib_amd.model.medplib import MedPLIBForCausalLM


def rate(model, device, new):
    cfg = model.config
    g = torch.Generator().manual_seed(0)
    L, V = 64, cfg.vocab_size
    ids = torch.randint(3, 31999, (1, L), generator=g)
    ids[0, 0] = 1; ids[0, 34], ids[0, 35], ids[0, 36] = V - 2, -200, V - 1
    images_clip = torch.randn(1, 3, 336, 336, generator=g).to(torch.bfloat16).to(device)
    images = torch.randn(1, 3, 256, 256, generator=g).to(device)
    model.evaluate(images_clip, images, ids.numpy(), [(256, 256)], [(336, 336)], max_new_tokens=8, eos_token_id=-1)
    res = {}
    for n_new in (new, 4 * new):
        best = float("inf")
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            model.evaluate(images_clip, images, ids.numpy(), [(256, 256)], [(336, 336)], max_new_tokens=n_new, eos_token_id=-1)
            torch.cuda.synchronize(); best = min(best, time.perf_counter() - t0)
        res[n_new] = best
    ms = (res[4 * new] - res[new]) / (3 * new) * 1e3
    d, ff, k = cfg.hidden_size, cfg.intermediate_size, cfg.top_k_experts
    wbytes = (cfg.num_hidden_layers * (4 * d * d + k * 3 * d * ff) + V * d) * 2
    return {"ms_per_token": round(ms, 3), "weight_bytes_per_token": wbytes, "weight_stream_GBps": round(wbytes / ms / 1e6, 1),
            "frac_of_8TBps": round(wbytes / (ms * 1e-3) / 8e12, 4), "path": getattr(model, "last_decode_path", None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cases = [("top1_E2_graph", dict(num_experts=2, top_k_experts=1), True),
             ("top2_E3_loop", dict(num_experts=3, top_k_experts=2), False),
             ("top2_E3_graph", dict(num_experts=3, top_k_experts=2), True)]
    out = {"metric": "decode ms/token (evaluate(), batch 1, KV cache, 32 MoE layers at 7B dims)", "new_tokens": [args.new, 4 * args.new]}
    model, built = None, None
    for name, kw, graph in cases:
        if built != kw:
            model = None
            gc.collect(); torch.cuda.empty_cache()
            model = MedPLIBForCausalLM(MedPLIBConfig.medplib_7b(moe_enable=True, **kw), device=dev).eval()
            built = kw
        model.decode_with_graph = graph
        out[name] = rate(model, dev, args.new)
        print(name, json.dumps(out[name]), flush=True)
    t1, tl, tg = out["top1_E2_graph"]["ms_per_token"], out["top2_E3_loop"]["ms_per_token"], out["top2_E3_graph"]["ms_per_token"]
    out["top2_graph_speedup_over_loop"] = round(tl / tg, 3)
    out["top2_graph_over_top1_graph"] = round(tg / t1, 3)
    d, ff, L = 4096, 11008, 32
    # what the extra expert's MLP stream alone would cost at the top-1 step's streaming rate
    extra = L * 3 * d * ff * 2 / (out["top1_E2_graph"]["weight_stream_GBps"] * 1e6)
    out["top2_graph_expected_ms_if_only_the_extra_expert_stream"] = round(t1 + extra, 3)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
