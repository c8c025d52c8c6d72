"""generate_batch() at the 7B dimensions: ragged prompts as the rows of one decode step against the same prompts through generate() one by
one, and — on the MoE model, with bf16 weights and under --w8 / --w4 alike — against the batch path with the indexed expert GEMVs
(MP_GEMV_GROUPED=0: one weight stream per row).
python scripts/batch_decode_bench.py [--dense | --top2] [--w8 | --w4] [--new 64] [--repeats 3] [--rows 1,2,4,8] [--gemv]
--top2: the 7B model with E = 3 experts, top-2 routing and moe_gate_sampling off (the reference's vqa_infer.py defaults minus the draws): the
batch path with the grouped top-2 pair (ops.gemv_grouped_top2_gate_up / _down) against the per-entry pair (group_expert_gemvs = False).

Prompts: B texts whose spliced lengths are spread over ~100 positions around 640 (576 image positions + 16..114 text tokens), eos -1.
Time: device events around the whole call, at 16 and at 16 + --new new tokens; the slope is the step time (prefill and the one-off graph
capture cancel out), tokens/s = B / step time.  The variants of one B alternate inside every repeat, in one process, after a warm-up of every
shape; every repeat is printed so that the spread shows.  One JSON line per (B, variant).
--gemv: the expert projections of one layer alone at B = 4 (two rows per expert), grouped against indexed, on the weights of the mode that is
on (bf16, --w8: int8 copies, --w4: NF4 copies): us per launch and bytes/s of the weights the launch has to read (both experts' matrices once).
--top2 --gemv: one layer's top-2 pair (gate|up + down) at E = 3 for B = 1, 2, 4, 8 (token t names experts t % 3 and (t + 1) % 3), grouped
against per-entry, alternating in one process, device events around each pair after a warm-up; beside the times the expected byte ratio from
the shapes alone: 2B weight streams against the number of distinct experts named."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from medplib_amd import ops
from medplib_amd.model.config import MedPLIBConfig
from medplib_amd.model.medplib import LISAForCausalLM, MedPLIBForCausalLM

ap = argparse.ArgumentParser()
ap.add_argument("--new", type=int, default=64)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--rows", default="1,2,4,8")
ap.add_argument("--dense", action="store_true")
ap.add_argument("--top2", action="store_true", help="E = 3, top-2 (a MoE batch: ops.gemv_grouped_top2_gate_up / _down)")
ap.add_argument("--pair_repeats", type=int, default=100, help="--top2 --gemv: timed pairs per (B, variant), at least")
ap.add_argument("--window_ms", type=float, default=600.0, help="--top2 --gemv: summed device time of the timed pairs of a variant, at least")
ap.add_argument("--w8", action="store_true", help="8-bit decode weights (a MoE batch: ops.gemv_grouped_w8)")
ap.add_argument("--w4", action="store_true", help="4-bit NF4 decode weights (a MoE batch: ops.gemv_grouped_w4)")
ap.add_argument("--gemv", action="store_true", help="only the expert GEMVs of one layer at B = 4, grouped against indexed")
args = ap.parse_args()
assert not (args.w8 and args.w4), "--w8 and --w4 are exclusive"
assert not (args.top2 and (args.dense or args.w8 or args.w4)), "--top2 is the bf16 MoE model (top-2 on the quantised copies is refused)"
dev = torch.device("cuda:0")
# (moe_gate_sampling off: generate_batch refuses the gate's random draws, which are keyed on the pass number and so on the prompts decoded before)
top2_cfg = dict(num_experts=3, top_k_experts=2) if args.top2 else {}
cfg = MedPLIBConfig.medplib_7b(moe_enable=not args.dense, moe_gate_sampling=False, **top2_cfg)
BASE = 16


def timed(fn):
    """Device time of fn() in ms (events on the current stream; fn ends synchronised)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


if args.gemv and args.top2:
    d, ff, E = cfg.hidden_size, cfg.intermediate_size, cfg.num_experts
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: (torch.randn(*s, generator=g, device=dev) * 0.02).to(torch.bfloat16)       # noqa: E731
    gu, down = rn(E, 2 * ff, d), rn(E, d, ff)
    mlp_bytes = (gu[0].numel() + down[0].numel()) * 2
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    for B in [int(x) for x in args.rows.split(",")]:
        h, x = rn(B, d), rn(B, d)
        first, second = [t % E for t in range(B)], [(t + 1) % E for t in range(B)]
        expert = torch.tensor(first + second, dtype=torch.int32, device=dev)
        slot = torch.arange(2 * B, dtype=torch.int32, device=dev)
        weight = torch.full((2 * B,), 0.5, dtype=torch.float32, device=dev)
        pairs = {
            "grouped": lambda: ops.gemv_grouped_top2_down(ops.gemv_grouped_top2_gate_up(h, gu, expert, slot), down, expert, slot, weight, x),
            "per-entry": lambda: ops.gemv_top2_down(ops.gemv_top2_gate_up(h, gu, expert, slot), down, expert, slot, weight, x),
        }
        assert torch.equal(pairs["grouped"](), pairs["per-entry"]())
        warm = [timed(fn) for _ in range(5) for fn in pairs.values()]
        # enough pairs for a timed window of args.window_ms per variant, sized by the faster one
        n_pairs = max(args.pair_repeats, int(args.window_ms / min(warm)) + 1)
        ts = {name: [] for name in pairs}
        for _ in range(n_pairs):
            for name, fn in pairs.items():            # the variants alternate
                flush.zero_()                         # (no launch finds its matrices in the cache)
                ts[name].append(timed(fn) * 1e3)
        distinct = len(set(first + second))
        med = {name: statistics.median(t) for name, t in ts.items()}
        for name, t in ts.items():
            q = statistics.quantiles(t, n=10)
            streams = distinct if name == "grouped" else 2 * B
            print(json.dumps({"pair": name, "B": B, "E": E, "entries": 2 * B, "experts_named": distinct, "us_median": round(med[name], 1),
                              "us_p10": round(q[0], 1), "us_p90": round(q[-1], 1), "timed_pairs": len(t), "window_ms": round(sum(t) / 1e3, 1),
                              "expert_mlps_streamed": streams, "TBps_of_those_bytes": round(streams * mlp_bytes / med[name] / 1e6, 2)}))
        print(json.dumps({"B": B, "per_entry_over_grouped_time": round(med["per-entry"] / med["grouped"], 3),
                          "expected_byte_ratio_from_shapes": round(2 * B / distinct, 3)}))
    sys.exit(0)

if args.gemv:
    d, ff, E = cfg.hidden_size, cfg.intermediate_size, cfg.num_experts
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: (torch.randn(*s, generator=g, device=dev) * 0.02).to(torch.bfloat16)       # noqa: E731
    gu, down = rn(E, 2 * ff, d), rn(E, d, ff)
    h, act_in, x = rn(4, d), rn(4, ff), rn(4, d)
    expert = torch.tensor([0, 1, 0, 1], dtype=torch.int32, device=dev)
    slot = torch.tensor([0, 0, 1, 1], dtype=torch.int32, device=dev)
    weight = torch.full((4,), 0.75, dtype=torch.float32, device=dev)
    if args.w8 or args.w4:                  # the mode's copies and its pair of ops (llama.DECODE_MODES)
        from medplib_amd.model.llama import DECODE_MODES
        mode = DECODE_MODES[8 if args.w8 else 4]
        quant, indexed, grouped = (getattr(ops, n) for n in (mode.quantizer, mode.gemv, mode.gemv_grouped))
        gu, down = quant(gu), quant(down)
    else:
        indexed, grouped, gu, down = ops.gemv, ops.gemv_grouped, (gu,), (down,)
    forms = {
        "gate|up grouped": lambda: grouped(h, *gu, expert, act=ops.ACT_SWIGLU_PAIR, row_keep=slot),
        "gate|up indexed": lambda: indexed(h, *gu, act=ops.ACT_SWIGLU_PAIR, w_index=expert, **({"row_keep": slot} if len(gu) > 1 else {})),
        "down grouped": lambda: grouped(act_in, *down, expert, residual=x, row_scale=weight, row_keep=slot),
        "down indexed": lambda: indexed(act_in, *down, residual=x, w_index=expert, row_scale=weight, row_keep=slot),
    }
    weight_bytes = lambda ws: sum(t.numel() * t.element_size() for t in ws)                       # noqa: E731  (codes + scales / absmax)
    # the other projection's weights are touched between two launches, so that no launch finds its matrices in the cache
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    for name, fn in forms.items():
        fn()
    for name, fn in forms.items():
        ts = []
        for _ in range(20):
            flush.zero_()
            ts.append(timed(fn) * 1e3)
        nbytes = weight_bytes(gu if name.startswith("gate") else down)
        us = statistics.median(ts)
        print(json.dumps({"launch": name, "w8": bool(args.w8), "w4": bool(args.w4), "rows": 4, "experts_named": 2, "us_median": round(us, 1), "us_min": round(min(ts), 1), "us_max": round(max(ts), 1),
                          "weight_bytes": nbytes, "TBps_of_those_bytes": round(nbytes / us / 1e6, 2)}))
    sys.exit(0)

model = (LISAForCausalLM if args.dense else MedPLIBForCausalLM)(cfg, device=dev).eval()
if args.w8:
    model.enable_decode_8bit(True)
if args.w4:
    model.enable_decode_4bit(True)
llm = model.model.llm
V = cfg.vocab_size
gen = torch.Generator().manual_seed(0)


def prompts(B):
    """B prompts with 16..114 text tokens around one image (spliced: 591..689 positions) -> padded ids, mask, images."""
    lengths = [int(round(x)) for x in np.linspace(16, 114, B)] if B > 1 else [64]
    width = max(lengths)
    ids, att = torch.zeros((B, width), dtype=torch.int64), torch.zeros((B, width), dtype=torch.bool)
    for r, L in enumerate(lengths):
        row = torch.randint(3, 31999, (L,), generator=gen)
        row[0] = 1
        row[8], row[9], row[10] = V - 2, -200, V - 1
        ids[r, :L], att[r, :L] = row, True
    return ids.numpy(), att.numpy(), torch.randn(B, 3, 336, 336, generator=gen).to(torch.bfloat16).to(dev), lengths


def run_batch(p, n_new, grouped):
    llm.group_expert_gemvs = grouped
    out = model.generate_batch(p[0], images=p[2], attention_mask=p[1], max_new_tokens=n_new, eos_token_id=-1, batch_rows=len(p[3]))
    assert out.shape[1] == max(p[3]) + n_new and model.last_decode_path == "graph"


def run_single(p, n_new):
    out = model.generate(p[0], images=p[2], attention_mask=p[1], max_new_tokens=n_new, eos_token_id=-1)
    assert out.shape[1] == max(p[3]) + n_new and model.last_decode_path == "graph"


for B in [int(x) for x in args.rows.split(",")]:
    p = prompts(B)
    variants = {"generate_batch": lambda n: run_batch(p, n, True), "generate() one by one": lambda n: run_single(p, n)}
    if not args.dense:
        variants["generate_batch, MP_GEMV_GROUPED=0"] = lambda n: run_batch(p, n, False)
    if args.top2:                                     # the question here is grouped against per-entry: no one-by-one arm
        del variants["generate() one by one"]
    for fn in variants.values():                      # warm-up of every shape
        fn(BASE)
    step_ms = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():             # the variants alternate inside a repeat
            short, long = timed(lambda: fn(BASE)), timed(lambda: fn(BASE + args.new))
            # one by one, the B prompts decode one after the other: the slope is the time of B steps
            step_ms[name].append((long - short) / args.new)
    for name, ts in step_ms.items():
        per_step = statistics.median(ts)
        tokens_per_step = B
        print(json.dumps({"B": B, "variant": name, "moe": not args.dense, "w8": bool(args.w8), "w4": bool(args.w4), "spliced_lengths": [n + 575 for n in p[3]],
                          "ms_per_step_of_B_tokens": round(per_step, 3), "tokens_per_s": round(tokens_per_step / per_step * 1e3, 1),
                          "repeats_ms": [round(t, 3) for t in ts]}))
    if args.top2:                                     # the criterion: faster than the off arm by more than the off arm's own spread
        on, off = step_ms["generate_batch"], step_ms["generate_batch, MP_GEMV_GROUPED=0"]
        spread = max(off) - min(off)
        entries = 2 * B
        print(json.dumps({"B": B, "off_arm_spread_ms": round(spread, 3), "off_minus_on_ms": round(statistics.median(off) - statistics.median(on), 3),
                          "faster_by_more_than_the_spread": statistics.median(off) - statistics.median(on) > spread,
                          "expected_byte_ratio_of_a_moe_layers_experts_at_most": round(entries / min(cfg.num_experts, entries), 3)}))
