"""Beam search at the 7B dimensions: ms per decode step of generate_beam(num_beams = 1, 2, 4, 8) beside the greedy step of generate(), dense
and E = 2 top-1, and the two beam kernels alone (the selection over nb x 32011 logits, the cache re-order at tails of 16, 64 and 512
generated tokens).  Protocol of scripts/decode_bench.py: one untimed call, then the slope between two answer lengths (--new and 4 x --new
tokens, the fastest of three calls each), so prefill and the one-off graph capture cancel out.  On a build without generate_beam (the parent
commit) only the greedy rows are measured: run the same command there to see that the greedy step has not moved.
python scripts/beam_bench.py [--new 16] [--kinds dense,top1] [--out profiles/beam_bench.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from medplib_amd import ops
from medplib_amd.model.config import MedPLIBConfig
from medplib_amd.model.medplib import LISAForCausalLM, MedPLIBForCausalLM

ap = argparse.ArgumentParser()
ap.add_argument("--new", type=int, default=16)
ap.add_argument("--kinds", default="dense,top1")
ap.add_argument("--beams", default="1,2,4,8")
ap.add_argument("--out", default="")
ap.add_argument("--w8", action="store_true", help="8-bit decode weights on (enable_decode_8bit) for the model steps")
ap.add_argument("--w4", action="store_true", help="4-bit NF4 decode weights on (enable_decode_4bit) for the model steps")
args = ap.parse_args()
assert not (args.w8 and args.w4), "--w8 and --w4 are exclusive"
dev = torch.device("cuda:0")
res = {"protocol": f"slope between {args.new} and {4 * args.new} generated tokens, fastest of 3 calls each, eos off", "steps": {}, "kernels": {},
       "decoder_weight_bytes_streamed_per_weight": 0.5625 if args.w4 else 1.0 if args.w8 else 2.0}     # NF4: half a byte + an fp32 absmax per 64


def event_ms(fn, iters):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


if hasattr(ops, "beam_topk"):
    g = torch.Generator().manual_seed(0)
    V = 32011
    for nb in (1, 2, 4, 8):
        logits = (torch.randn(nb, V, generator=g) * 3).to(dev)
        scores = -torch.rand(nb, generator=g).to(dev)
        cs, ci = torch.empty(2 * nb, device=dev), torch.empty(2 * nb, dtype=torch.int32, device=dev)
        ns, nt, npar = torch.empty(nb, device=dev), torch.empty(nb, dtype=torch.int64, device=dev), torch.empty(nb, dtype=torch.int32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        res["kernels"][f"beam_topk nb={nb} cols={V} us"] = round(1e3 * event_ms(lambda: ops.beam_topk(logits, scores, 2, cs, ci, ns, nt, npar, err), 200), 2)
    # the 7B cache: 32 layers x (K, V) [nb, S + tail, 32, 128] bf16, S = 64 prompt rows that never move; a full cycle of parents moves every row
    S, nb = 64, 8
    for tail in (16, 64, 512):
        cache = [torch.zeros((nb, S + tail, 32, 128), dtype=torch.bfloat16, device=dev) for _ in range(64)]
        table, _ = ops.kv_permute_table(cache)
        par = torch.tensor([(b + 1) % nb for b in range(nb)], dtype=torch.int32, device=dev)
        hi, err = torch.tensor([S + tail], dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        ms = event_ms(lambda: ops.kv_permute_rows(table, cache[0], par, S, hi, err), 50)
        moved = 2 * 64 * nb * tail * 4096 * 2                   # read + written
        res["kernels"][f"kv_permute_rows nb={nb} tail={tail}"] = {"us": round(1e3 * ms, 2), "bytes_moved": moved, "GBps": round(moved / ms / 1e6, 1)}
        del cache, table
    print(json.dumps(res["kernels"]), flush=True)

g = torch.Generator().manual_seed(0)
for kind in args.kinds.split(","):
    dense = kind == "dense"
    cfg = MedPLIBConfig.medplib_7b(moe_enable=False) if dense else MedPLIBConfig.medplib_7b(moe_enable=True, num_experts=2, top_k_experts=1)
    model = (LISAForCausalLM if dense else MedPLIBForCausalLM)(cfg, device=dev).eval()
    if args.w8:
        model.enable_decode_8bit(True)
    if args.w4:
        model.enable_decode_4bit(True)
    L, V = 64, cfg.vocab_size
    ids = torch.randint(3, 31999, (1, L), generator=g)
    ids[0, 0] = 1; ids[0, 34], ids[0, 35], ids[0, 36] = V - 2, -200, V - 1
    clip = torch.randn(1, 3, 336, 336, generator=g).to(torch.bfloat16).to(dev)

    def slope(call):
        call(8)                                  # untimed: code objects and other first-use costs
        best = {}
        for n_new in (args.new, 4 * args.new):
            best[n_new] = float("inf")
            for _ in range(3):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                out = call(n_new)
                torch.cuda.synchronize(); best[n_new] = min(best[n_new], time.perf_counter() - t0)
                assert out.shape[1] == L + n_new and model.last_decode_path == "graph"
        return round((best[4 * args.new] - best[args.new]) / (3 * args.new) * 1e3, 4)

    row = {"greedy generate() ms/step": slope(lambda n: model.generate(ids.numpy(), images=clip, max_new_tokens=n, eos_token_id=-1))}
    if hasattr(model, "generate_beam"):
        for nb in (int(x) for x in args.beams.split(",")):
            row[f"generate_beam(num_beams={nb}) ms/step"] = slope(
                lambda n: model.generate_beam(ids.numpy(), images=clip, max_new_tokens=n, eos_token_id=-1, num_beams=nb))
        # the greedy step again, after the beam runs: the spread of the same measurement inside this process
        row["greedy generate() ms/step, again"] = slope(lambda n: model.generate(ids.numpy(), images=clip, max_new_tokens=n, eos_token_id=-1))
    res["steps"][kind] = row
    print(json.dumps({kind: row}), flush=True)
    del model
    torch.cuda.empty_cache()

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
