"""generate_sample_batch() / generate_stream_batch() at the 7B dimensions: requests that sample differently as the rows of one decode step.
python scripts/sample_batch_bench.py [--new 32] [--repeats 3] [--rows 1,2,4,5,8] [--models dense,moe] [--out profiles/sample_batch.json]

Models: dense, and E = 2 top-1 without gate sampling (the batch rows refuse the gate's draws), random weights.  Prompts: B texts whose spliced
lengths are spread over ~100 positions around 640 (scripts/batch_decode_bench.py's), eos -1.  The rows cycle through three kinds of request:
top_k = 1 (HF's way to ask a sampler for the argmax), T = 0.2 / top_k = 50 / top_p = 0.9, and T = 1 plain (no filter); the stream arm asks
for the first kind as temperature = 0, a truly greedy row of the per-row pick.
  (a) tokens/s of generate_sample_batch against the same prompts and parameters one by one through generate_sample (row b under seed + b in
      both): what one process could do before;
  (b) ms per step of generate_sample_batch and of generate_stream_batch against generate_batch's greedy step at the same B: what the draw
      and the per-row pick cost.  The bar: below B times the single-row cost of sampling — generate_stream's ms per token with the filtered
      pick (k = 50, p = 0.9) minus greedy, measured here on the same model in the same process, scripts/sample_filtered_bench.py's protocol
      with a greedy arm added — since B separate picks would cost that much.
Time: device events around the whole call at 16 and at 16 + --new new tokens; the slope is the step time (prefills and the one-off graph
capture cancel out).  The arms of one B alternate inside every repeat, in one process, after a warm-up of every shape; every repeat is
printed so that the spread shows.  One JSON line per (model, B, arm)."""
import argparse
import gc
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from medplib_amd.model.config import MedPLIBConfig
from medplib_amd.model.generation import StreamRequest
from medplib_amd.model.medplib import LISAForCausalLM, MedPLIBForCausalLM

BASE, SEED = 16, 7
KINDS = ((0.7, 1, 1.0), (0.2, 50, 0.9), (1.0, 0, 1.0))      # (temperature, top_k, top_p); the first is the argmax


def timed(fn):
    """Device time of fn() in ms (events on the current stream; fn ends synchronised)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def prompts(B, V, gen, dev):
    """B prompts with 16..114 text tokens around one image (spliced: 591..689 positions) -> padded ids, mask, images, lengths."""
    lengths = [int(round(x)) for x in np.linspace(16, 114, B)] if B > 1 else [64]
    width = max(lengths)
    ids, att = torch.zeros((B, width), dtype=torch.int64), torch.zeros((B, width), dtype=torch.bool)
    for r, L in enumerate(lengths):
        row = torch.randint(3, 31999, (L,), generator=gen)
        row[0] = 1
        row[8], row[9], row[10] = V - 2, -200, V - 1
        ids[r, :L], att[r, :L] = row, True
    return ids.numpy(), att.numpy(), torch.randn(B, 3, 336, 336, generator=gen).to(torch.bfloat16).to(dev), lengths


def slopes(arms, new, repeats):
    """{name: fn(n_new)} -> {name: [ms per step, one per repeat]}; the arms alternate inside a repeat."""
    for fn in arms.values():                          # warm-up of every shape
        fn(BASE)
    out = {name: [] for name in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            short, long = timed(lambda: fn(BASE)), timed(lambda: fn(BASE + new))
            out[name].append((long - short) / new)
    return out


def single_row_cost(model, p, new, repeats):
    """generate_stream on one ~640-position prompt: ms per token greedy, plain (T = 1) and filtered (T = 0.2, k = 50, p = 0.9)."""
    ids, clip = p[0][:1, :p[3][0]], p[2][:1]

    def run(n_new, **kw):
        for _ in model.generate_stream(ids, clip, max_new_tokens=n_new, eos_token_id=-1, stream_interval=16, sample_seed=SEED, **kw):
            pass
        assert model.last_decode_path == "graph"

    arms = {"greedy": lambda n: run(n, temperature=0.0), "plain": lambda n: run(n, temperature=1.0),
            "filtered": lambda n: run(n, temperature=0.2, top_k=50, top_p=0.9, apply_top_p=True)}
    ts = slopes(arms, new, repeats)
    med = {k: statistics.median(v) for k, v in ts.items()}
    return {"ms_per_token": {k: round(v, 4) for k, v in med.items()}, "repeats_ms": {k: [round(t, 4) for t in v] for k, v in ts.items()},
            "plain_minus_greedy_us": round((med["plain"] - med["greedy"]) * 1e3, 1),
            "filtered_minus_greedy_us": round((med["filtered"] - med["greedy"]) * 1e3, 1)}


def bench_model(name, model, dev, args, out):
    V = model.config.vocab_size
    gen = torch.Generator().manual_seed(0)
    single = single_row_cost(model, prompts(1, V, gen, dev), args.new, args.repeats)
    out[name] = {"single_row": single, "rows": {}}
    print(json.dumps({"model": name, "single_row": single}), flush=True)
    cost = {0: 0.0, 1: single["filtered_minus_greedy_us"], 2: single["plain_minus_greedy_us"]}     # per kind of row, us
    for B in [int(x) for x in args.rows.split(",")]:
        p = prompts(B, V, gen, dev)
        kinds = [KINDS[r % 3] for r in range(B)]
        T, K, P = [k[0] for k in kinds], [k[1] for k in kinds], [k[2] for k in kinds]

        def sample_batch(n):
            o = model.generate_sample_batch(p[0], images=p[2], attention_mask=p[1], max_new_tokens=n, eos_token_id=-1, temperature=T, top_k=K,
                                            top_p=P, sample_seed=SEED, batch_rows=B)
            assert o.shape[1] == max(p[3]) + n and model.last_decode_path == "graph"

        def one_by_one(n):
            for b in range(B):
                model.generate_sample(p[0][b:b + 1], images=p[2][b:b + 1], attention_mask=p[1][b:b + 1], max_new_tokens=n, eos_token_id=-1,
                                      temperature=T[b], top_k=K[b], top_p=P[b], sample_seed=SEED + b)
                assert model.last_decode_path == "graph"

        def greedy_batch(n):
            o = model.generate_batch(p[0], images=p[2], attention_mask=p[1], max_new_tokens=n, eos_token_id=-1, batch_rows=B)
            assert o.shape[1] == max(p[3]) + n and model.last_decode_path == "graph"

        def stream_batch(n):
            reqs = [StreamRequest(input_ids=p[0][b:b + 1, :p[3][b]], images_clip=p[2][b:b + 1], temperature=0.0 if b % 3 == 0 else T[b],
                                  top_k=K[b], top_p=P[b], apply_top_p=True, max_new_tokens=n, sample_seed=SEED + b) for b in range(B)]
            for _ in model.generate_stream_batch(reqs, stream_interval=16, eos_token_id=-1):
                pass
            assert model.last_decode_path == "graph"

        arms = {"generate_sample_batch": sample_batch, "generate_sample one by one": one_by_one, "generate_batch (greedy)": greedy_batch,
                "generate_stream_batch": stream_batch}
        ts = slopes(arms, args.new, args.repeats)
        med = {k: statistics.median(v) for k, v in ts.items()}
        bar_b_times = B * single["filtered_minus_greedy_us"]
        bar_by_kind = sum(cost[r % 3] for r in range(B))
        res = {"spliced_lengths": [n + 575 for n in p[3]], "kinds": kinds,
               "ms_per_step": {k: round(v, 4) for k, v in med.items()}, "repeats_ms": {k: [round(t, 4) for t in v] for k, v in ts.items()},
               "tokens_per_s": {k: round(B / med[k] * 1e3, 1) for k in ("generate_sample_batch", "generate_sample one by one")},
               "excess_over_greedy_step_us": {k: round((med[k] - med["generate_batch (greedy)"]) * 1e3, 1)
                                              for k in ("generate_sample_batch", "generate_stream_batch")},
               "greedy_step_spread_us": round((max(ts["generate_batch (greedy)"]) - min(ts["generate_batch (greedy)"])) * 1e3, 1),
               "bar_B_times_single_row_filtered_us": round(bar_b_times, 1), "bar_sum_of_each_rows_own_single_row_cost_us": round(bar_by_kind, 1)}
        res["below_bar"] = {k: v < bar_b_times for k, v in res["excess_over_greedy_step_us"].items()}
        out[name]["rows"][str(B)] = res
        print(json.dumps({"model": name, "B": B, **res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rows", default="1,2,4,5,8")
    ap.add_argument("--models", default="dense,moe")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"script": "python scripts/sample_batch_bench.py --new %d --repeats %d --rows %s --models %s" % (args.new, args.repeats, args.rows, args.models),
           "metric": "ms per decode step of B rows (captured graph, 7B dims, prompts of 591..689 spliced positions), slope between %d and %d new "
                     "tokens; single_row: generate_stream ms per token at batch 1" % (BASE, BASE + args.new),
           "kinds_of_rows_cycled": [list(k) for k in KINDS]}
    for name, cls, moe in (("dense", LISAForCausalLM, False), ("moe", MedPLIBForCausalLM, True)):
        if name not in args.models.split(","):
            continue
        # (moe_gate_sampling off: batch rows refuse the gate's random draws, which are keyed on the pass number)
        model = cls(MedPLIBConfig.medplib_7b(moe_enable=moe, moe_gate_sampling=False), device=dev).eval()
        bench_model(name, model, dev, args, out)
        model = None
        gc.collect(); torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
