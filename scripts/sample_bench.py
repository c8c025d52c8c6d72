"""What temperature sampling costs on the device (generate_stream):
  1. microseconds per launch of mp_sample_rows_f32 against mp_argmax_rows_f32 on a [1, 32000] fp32 row — 200 launches captured into one HIP
     graph and replayed, so the figure is the device's back-to-back time without the host's launch cost; the same on a [1, 40000] row,
     past the 32768 columns up to which the pick kernels hold the row in registers;
  2. milliseconds per token of the captured decode step with the sampling pick (draw + mp_sample_rows_f32) against the greedy pick (argmax),
     dense and MoE at bench.py's decode configuration (7B dims, batch 1, 64-token prompt): generate_stream's slope between two lengths
     (bench.py decode_rate's method: prefill and the graph capture cancel; the fastest of three calls per length after one untimed call),
     the two picks measured alternately in the same process on the same model.
python scripts/sample_bench.py [--new 32] [--out profiles/sample_bench.json]"""
import argparse
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from medplib_amd import ops
from medplib_amd.model.config import MedPLIBConfig
from medplib_amd.model.medplib import LISAForCausalLM, MedPLIBForCausalLM


def kernel_us(dev, cols=32000, launches=200, replays=20):
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(1, cols, generator=g) * 2).to(dev)
    u = torch.tensor([0.37], device=dev)
    out = {}
    for name, fn in (("argmax_rows", lambda: ops.argmax_rows(logits)), ("sample_rows", lambda: ops.sample_rows(logits, u, 0.7))):
        fn(); torch.cuda.synchronize()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                for _ in range(launches):
                    fn()
        torch.cuda.current_stream().wait_stream(side)
        graph.replay(); torch.cuda.synchronize()
        best = float("inf")
        for _ in range(replays):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); graph.replay(); b.record(); torch.cuda.synchronize()
            best = min(best, a.elapsed_time(b))
        out[name] = round(best * 1e3 / launches, 3)
    out["sample_over_argmax"] = round(out["sample_rows"] / out["argmax_rows"], 3)
    return out


def step_ms(model, dev, new):
    cfg = model.config
    g = torch.Generator().manual_seed(0)
    L, V = 64, cfg.vocab_size
    ids = torch.randint(3, 31999, (1, L), generator=g)
    ids[0, 0] = 1; ids[0, 34], ids[0, 35], ids[0, 36] = V - 2, -200, V - 1
    clip = torch.randn(1, 3, 336, 336, generator=g).to(torch.bfloat16).to(dev)

    def run(T, n_new):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in model.generate_stream(ids.numpy(), clip, temperature=T, max_new_tokens=n_new, eos_token_id=-1, stream_interval=16):
            pass
        torch.cuda.synchronize()
        assert model.last_decode_path == "graph"
        return time.perf_counter() - t0

    picks = {"greedy": 0.0, "sampling": 0.7}
    for T in picks.values():
        run(T, 8)
    best = {(k, n): float("inf") for k in picks for n in (new, 4 * new)}
    for _ in range(3):
        for n_new in (new, 4 * new):
            for k, T in picks.items():                   # alternately: a drift of the box hits both picks alike
                best[(k, n_new)] = min(best[(k, n_new)], run(T, n_new))
    res = {k: round((best[(k, 4 * new)] - best[(k, new)]) / (3 * new) * 1e3, 4) for k in picks}
    res["sampling_over_greedy"] = round(res["sampling"] / res["greedy"], 4)
    res["sampling_minus_greedy_us"] = round((res["sampling"] - res["greedy"]) * 1e3, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"script": "python scripts/sample_bench.py --new %d" % args.new,
           "kernel_us_per_launch_1x32000": kernel_us(dev),
           "kernel_us_per_launch_1x40000": kernel_us(dev, cols=40000),       # past 32768 columns: the kernels that read the row again
           "metric": "decode ms/token (generate_stream, captured graph, batch 1, KV cache, 7B dims, stream_interval 16)",
           "new_tokens": [args.new, 4 * args.new]}
    print(json.dumps(out["kernel_us_per_launch_1x32000"]), json.dumps(out["kernel_us_per_launch_1x40000"]), flush=True)
    for name, cls, moe in (("dense", LISAForCausalLM, False), ("moe", MedPLIBForCausalLM, True)):
        model = cls(MedPLIBConfig.medplib_7b(moe_enable=moe), device=dev).eval()
        out[name] = step_ms(model, dev, args.new)
        print(name, json.dumps(out[name]), flush=True)
        model = None
        gc.collect(); torch.cuda.empty_cache()
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
