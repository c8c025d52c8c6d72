"""Decoding with LoRA adapters attached, at the 7B layer dimensions with 4 decoder layers: what the shadow merge costs and whether the decode
that follows is the merged model's.  Three configurations (the shipped scripts' stages):
    stage3   MoE E = 2 top-1, adapters on the experts' gate / up / down_proj, r = 8
    stage4   the same plus q_proj, v_proj
    stage2   dense, all seven targets, r = 16
Per configuration: the time of LoRAState.merge_shadow (all of it, and its one mp_lora_merge_rows_batched launch alone) and of restore_plain
(HIP events, median of --reps after warm-up), the bytes each moves and the fraction of the 6.29 TB/s a device copy reaches; the time of
LoRAState.merge_into (the torch merge behind merge_and_unload(): per adapter an fp32 B @ A, a gather / add / cast / scatter over the rows, then
the copies it refreshes) on the same adapters; and ms per token of a greedy decode (evaluate(), the slope between 16 and 16 + --new new
tokens, --decode-reps times) with the adapters live inside an adapters_merged() block (twice: before and after the merge timings, which
shows how far two blocks of the SAME model drift apart), beside the same model after merge_and_unload().
python scripts/adapter_merge_bench.py [--new 64] [--reps 20] [--out FILE]"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from medplib_amd import ops
from medplib_amd.model.config import MedPLIBConfig
from medplib_amd.model.llama_lora import GROUPS
from medplib_amd.model.medplib import LISAForCausalLM, MedPLIBForCausalLM

COPY_BPS = 6.29e12
CASES = {
    "stage3": dict(moe=True, r=8, alpha=16, targets="gate_proj,up_proj,down_proj"),
    "stage4": dict(moe=True, r=8, alpha=16, targets="q_proj,v_proj,gate_proj,up_proj,down_proj"),
    "stage2": dict(moe=False, r=16, alpha=32, targets="q_proj,k_proj,v_proj,o_proj,gate_proj,up_proj,down_proj"),
}


def event_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record(); e.synchronize()
        ts.append(s.elapsed_time(e))
    return ts


def decode_ms(model, dev, new, reps):
    """ms per decode step, `reps` times: (evaluate at 16 + new tokens) - (evaluate at 16 tokens), each the faster of two calls."""
    cfg = model.config
    g = torch.Generator().manual_seed(0)
    V = cfg.vocab_size
    ids = torch.randint(3, 31999, (1, 64), generator=g)
    ids[0, 0] = 1; ids[0, 34], ids[0, 35], ids[0, 36] = V - 2, -200, V - 1
    clip = torch.randn(1, 3, 336, 336, generator=g).to(torch.bfloat16).to(dev)
    sam = torch.randn(1, 3, 256, 256, generator=g).to(dev)

    def run(n):
        best = float("inf")
        for _ in range(2):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            model.evaluate(clip, sam, ids.numpy(), [(256, 256)], [(336, 336)], max_new_tokens=n, eos_token_id=-1)
            torch.cuda.synchronize(); best = min(best, time.perf_counter() - t0)
        return best
    run(8)
    return [round((run(16 + new) - run(16)) / new * 1e3, 4) for _ in range(reps)]


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def one(name, spec, dev, args):
    kw = dict(num_hidden_layers=4)
    if spec["moe"]:
        model = MedPLIBForCausalLM(MedPLIBConfig.medplib_7b(moe_enable=True, num_experts=2, top_k_experts=1, **kw), device=dev).eval()
    else:
        model = LISAForCausalLM(MedPLIBConfig.medplib_7b(moe_enable=False, **kw), device=dev).eval()
    lora = model.enable_lora(lora_r=spec["r"], lora_alpha=spec["alpha"], lora_dropout=0.0, lora_target_modules=spec["targets"])
    g = torch.Generator().manual_seed(1)
    for n, p in zip(lora.names, lora.params):
        if "lora_B" in n:
            p.data.copy_((0.02 * torch.randn(p.shape, generator=g)).to(dev))
    llm = model.model.llm
    res = {"adapters": sum("lora_A" in n for n in lora.names)}
    # bytes: the merge reads and writes the adapted rows once (2 + 2 bytes per element) and reads the fp32 masters; the restore copies whole groups
    rows_elems = sum(p.shape[0] * lora.params[lora.index[n.replace("lora_B", "lora_A")]].shape[1] for n, p in zip(lora.names, lora.params) if "lora_B" in n)
    master_bytes = 4 * sum(p.numel() for n, p in zip(lora.names, lora.params) if "lora_" in n)
    adapted = [k for k, mem in GROUPS.items() if any(t in lora.targets for t in mem)]
    group_elems = sum(lw[k].numel() for lw in llm.layers for k in adapted)
    res["merge_kernel_bytes"], res["restore_bytes"] = 4 * rows_elems + master_bytes, 4 * group_elems

    with model.adapters_merged():
        res["live_ms_per_token_first"] = decode_ms(model, dev, args.new, args.decode_reps)
    lora.merge_shadow(llm)
    t = event_ms(lambda: ops.lora_merge_rows_batched(lora._shadow_tab, lora._shadow_n), args.reps)
    res["merge_kernel_ms"] = spread(t)
    res["merge_kernel_frac_of_copy"] = round(res["merge_kernel_bytes"] / (statistics.median(t) * 1e-3) / COPY_BPS, 4)
    res["merge_shadow_ms"] = spread(event_ms(lambda: lora.merge_shadow(llm), args.reps))
    t = event_ms(lambda: lora.restore_plain(llm), args.reps)
    res["restore_plain_ms"] = spread(t)
    res["restore_frac_of_copy"] = round(res["restore_bytes"] / (statistics.median(t) * 1e-3) / COPY_BPS, 4)
    res["refreshes_qkv_rope"] = bool(llm.fuse_rope and any(t_ in GROUPS["qkv"] for t_ in lora.targets))

    with model.adapters_merged():
        res["live_ms_per_token"] = decode_ms(model, dev, args.new, args.decode_reps)
    res["path"] = model.last_decode_path
    # the torch merge on the same adapters (it accumulates into the weights: timed last, just before the model is merged for good)
    res["merge_into_ms"] = spread(event_ms(lambda: lora.merge_into(llm), max(3, args.reps // 4), warm=1))
    model.merge_and_unload()
    res["merged_ms_per_token"] = decode_ms(model, dev, args.new, args.decode_reps)
    res["live_first_ms"], res["live_ms"], res["merged_ms"] = spread(res["live_ms_per_token_first"]), spread(res["live_ms_per_token"]), spread(res["merged_ms_per_token"])
    res["shadow_over_merge_into"] = round(res["merge_shadow_ms"]["median"] / res["merge_into_ms"]["median"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--decode-reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="one of " + ", ".join(CASES))
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"metric": "shadow merge / restore (ms, HIP events) and decode ms/token with live adapters vs merged, 7B dims, 4 layers",
           "copy_rate_Bps": COPY_BPS, "new_tokens": args.new}
    for name, spec in CASES.items():
        if args.only and name != args.only:
            continue
        gc.collect(); torch.cuda.empty_cache()
        out[name] = one(name, spec, dev, args)
        print(name, json.dumps(out[name]), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
