"""The prefill of a generate_batch() group at the 7B dimensions: one padded pass (batch_prefill=True: LlamaStack.forward(seg_lens=), every MoE
layer routing each prompt as a pass of its own) against a prefill per row, on three models — dense, E = 2 top-1, E = 3 top-2 (the MoE
models with moe_gate_sampling off: batch rows refuse gate draws).
python scripts/batch_prefill_bench.py [--models dense,top1,top2] [--rows 1,2,4,8] [--repeats 5] [--new 64]

Prompts: those of scripts/batch_decode_bench.py — B texts whose spliced lengths are spread over ~100 positions around 640 (576 image
positions + 16..114 text tokens), eos -1.
Time: device events around _prefill_batch alone (planning, CLIP tower and splice included: both arms pay them per prompt), and around the
whole generate_batch(max_new_tokens=--new) call, per-row against batched.  The two arms alternate inside every repeat, in one process, after
a warm-up of every shape; every repeat is printed so that the spread shows.  One JSON line per (model, B, arm), and per (model, B) the
criterion: batched faster than per-row by more than the spread of the per-row arm's own repeats.  A group of one takes the per-row path
in both arms (B = 1 is the noise floor of the comparison)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from medplib_amd.model import generation as G
from medplib_amd.model.config import MedPLIBConfig
from medplib_amd.model.medplib import LISAForCausalLM, MedPLIBForCausalLM

ap = argparse.ArgumentParser()
ap.add_argument("--models", default="dense,top1,top2")
ap.add_argument("--rows", default="1,2,4,8")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--new", type=int, default=64)
args = ap.parse_args()
assert args.repeats >= 5, "at least 5 repeats: the criterion is the per-row arm's own spread"
dev = torch.device("cuda:0")
MODELS = {"dense": dict(moe_enable=False), "top1": dict(moe_enable=True, num_experts=2, top_k_experts=1),
          "top2": dict(moe_enable=True, num_experts=3, top_k_experts=2)}
ARMS = (("per-row", False), ("batched", True))


def timed(fn):
    """Device time of fn() in ms (events on the current stream; fn ends synchronised)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def prompts(B, V, gen):
    """B prompts with 16..114 text tokens around one image (spliced: 591..689 positions) -> padded ids, mask, images, text lengths."""
    lengths = [int(round(x)) for x in np.linspace(16, 114, B)] if B > 1 else [64]
    width = max(lengths)
    ids, att = torch.zeros((B, width), dtype=torch.int64), torch.zeros((B, width), dtype=torch.bool)
    for r, L in enumerate(lengths):
        row = torch.randint(3, 31999, (L,), generator=gen)
        row[0] = 1
        row[8], row[9], row[10] = V - 2, -200, V - 1
        ids[r, :L], att[r, :L] = row, True
    return ids.numpy(), att.numpy(), torch.randn(B, 3, 336, 336, generator=gen).to(torch.bfloat16).to(dev), lengths


for name in args.models.split(","):
    cfg = MedPLIBConfig.medplib_7b(moe_gate_sampling=False, **MODELS[name])
    model = (MedPLIBForCausalLM if cfg.moe_enable else LISAForCausalLM)(cfg, device=dev).eval()
    gen = torch.Generator().manual_seed(0)
    for B in [int(x) for x in args.rows.split(",")]:
        p = prompts(B, cfg.vocab_size, gen)
        group = [G._row_prompt(p[0].astype(np.int64), p[2], p[1], {}, b) for b in range(B)]

        def prefill(batched):
            with model._decoding("bench"):
                model._prefill_batch(group, args.new, batched=batched)

        def whole(batched):
            out = model.generate_batch(p[0], images=p[2], attention_mask=p[1], max_new_tokens=args.new, eos_token_id=-1, batch_rows=B,
                                       batch_prefill=batched)
            assert out.shape[1] == max(p[3]) + args.new and model.last_decode_path == "graph"

        for _, batched in ARMS:                           # warm-up of every shape
            prefill(batched)
            whole(batched)
        ms = {(what, arm): [] for what in ("prefill", "whole") for arm, _ in ARMS}
        for _ in range(args.repeats):
            for arm, batched in ARMS:                     # the arms alternate inside a repeat
                ms["prefill", arm].append(timed(lambda: prefill(batched)))
            for arm, batched in ARMS:
                ms["whole", arm].append(timed(lambda: whole(batched)))
        for arm, _ in ARMS:
            print(json.dumps({"model": name, "B": B, "arm": arm, "spliced_lengths": [n + 575 for n in p[3]],
                              "prefill_ms_median": round(statistics.median(ms["prefill", arm]), 2),
                              "prefill_ms_repeats": [round(t, 2) for t in ms["prefill", arm]],
                              f"generate_batch_{args.new}_ms_median": round(statistics.median(ms["whole", arm]), 2),
                              f"generate_batch_{args.new}_ms_repeats": [round(t, 2) for t in ms["whole", arm]]}), flush=True)
        row, bat = ms["prefill", "per-row"], ms["prefill", "batched"]
        spread = max(row) - min(row)
        gain = statistics.median(row) - statistics.median(bat)
        print(json.dumps({"model": name, "B": B, "per_row_spread_ms": round(spread, 2), "per_row_minus_batched_ms": round(gain, 2),
                          "per_row_over_batched": round(statistics.median(row) / statistics.median(bat), 3),
                          "faster_by_more_than_the_spread": gain > spread}), flush=True)
    del model
    torch.cuda.empty_cache()
