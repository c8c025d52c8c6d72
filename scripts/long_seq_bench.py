"""Long sequences on one MI355X: the 32-layer 7B decoder prefill (E = 2 top-1 MoE, B = 1) at S = 2048 / 4096 / 8192 with attention's share,
attention forward / backward TFLOP/s at those S next to S = 639 (B = 8), the LoRA stage-III step (per-GPU batch 8) at S = 2048, and graph
decode ms/token at cache positions ~700 and ~8000.  Writes one JSON object to --out (and stdout).
python scripts/long_seq_bench.py --out profiles/long_seq_bench.json"""
import argparse
import json
import os
import socket
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from medplib_amd import engine, ops
from medplib_amd.model.config import MedPLIBConfig
from medplib_amd.model.medplib import LISAForCausalLM, MedPLIBForCausalLM

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/long_seq_bench.json")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--skip", default="", help="comma list of legs to skip: prefill,attn,lora,decode")
args = ap.parse_args()
skip = set(filter(None, args.skip.split(",")))
dev = torch.device("cuda:0")
res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "reps": args.reps}


def timed(fn, reps, warmup=2):
    """Median and min ms of `reps` calls, each between device synchronisations (HIP events)."""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts))


def attn_flop(B, H, S, D, bwd=False):
    """Causal: half of the S x S products; forward 2 matmuls, backward 5 (with the recomputed QK^T)."""
    return B * H * S * S * D * 2 * (5 if bwd else 2) / 2


H, D = 32, 128
if "attn" not in skip:
    rows = []
    for B, S in ((8, 639), (1, 2048), (1, 4096), (1, 8192)):
        g = torch.Generator(device=dev).manual_seed(S)
        qkv = torch.randn(B, S, 3, H, D, generator=g, device=dev).to(torch.bfloat16)
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
        f_ms, f_min = timed(lambda: ops.attention(q, k, v, causal=True), args.reps * 4)
        out, lse = ops.attention_fwd_lse(q, k, v, causal=True)
        d_out = torch.randn_like(out)
        b_ms, b_min = timed(lambda: ops.attention_bwd(q, k, v, out, d_out, lse, causal=True), args.reps * 4)
        rows.append({"B": B, "S": S, "fwd_ms": round(f_ms, 3), "fwd_tflops": round(attn_flop(B, H, S, D) / f_ms / 1e9, 1),
                     "bwd_ms": round(b_ms, 3), "bwd_tflops": round(attn_flop(B, H, S, D, True) / b_ms / 1e9, 1),
                     "fwd_min_ms": round(f_min, 3), "bwd_min_ms": round(b_min, 3)})
        print(rows[-1], flush=True)
        del qkv, out, lse, d_out
    res["attention_H32_D128"] = rows

if "prefill" not in skip:
    cfg = MedPLIBConfig.medplib_7b(moe_enable=True)
    from medplib_amd.model.llama import LlamaStack
    st = LlamaStack(cfg, dev, seed=0)
    st.training = False
    rows = []
    with torch.no_grad():
        for S in (2048, 4096, 8192):
            emb = (torch.randn(1, S, cfg.hidden_size, device=dev) * 0.5).to(torch.bfloat16)
            ms, mn = timed(lambda: st.forward(emb, None), args.reps)
            qkv = torch.randn(1, S, 3, H, D, device=dev).to(torch.bfloat16)
            a_ms, _ = timed(lambda: ops.attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], causal=True), args.reps * 4)
            attn_total = a_ms * cfg.num_hidden_layers
            rows.append({"S": S, "prefill_ms": round(ms, 2), "prefill_min_ms": round(mn, 2), "attention_ms_32_layers": round(attn_total, 2),
                         "attention_share": round(attn_total / ms, 3), "rope_rows": int(st.cos.shape[0])})
            print(rows[-1], flush=True)
            del emb, qkv
    res["prefill_7b_32_layers_moe_e2_b1"] = rows
    del st
    torch.cuda.empty_cache()


def long_batch(cfg, B, S, seed):
    """bench.synthetic_batch with the prompt lengthened so that the spliced sequence has S positions (576 image tokens - 1 placeholder)."""
    b = bench.synthetic_batch(cfg, B, dev, seed)
    L = S - 575
    g = torch.Generator().manual_seed(seed)
    ids = np.asarray(torch.randint(3, 31999, (B, L), generator=g).numpy())
    ids[:, :64] = b["input_ids"][:, :64]
    ids[:, 61], ids[:, 63] = 3, 3                          # the <SEG> / EOS of the 64-token prompt move to the end
    ids[:, L - 3], ids[:, L - 1] = cfg.seg_token_idx, 2
    labels = ids.copy()
    labels[:, :L - 8] = -100
    b.update(input_ids=ids, labels=labels, attention_mask=np.ones((B, L), dtype=bool))
    return b


if "lora" not in skip:
    cfg = MedPLIBConfig.medplib_7b(moe_enable=False)
    model = LISAForCausalLM(cfg, device=dev).train()
    lora = model.enable_lora(lora_r=8, lora_alpha=16, lora_dropout=0.05, lora_target_modules="gate_proj,up_proj,down_proj",
                             sft_modules="mask_decoder,text_hidden_fcs")
    for n, p in zip(lora.names, lora.params):
        if "lora_B" in n:
            p.data.normal_(0, 0.01)
    eng, _, _, _ = engine.initialize(model=model, model_parameters=model.trainable_parameters(),
                                     config={"train_micro_batch_size_per_gpu": 8, "optimizer": {"params": {"lr": 1e-4, "betas": (0.9, 0.95)}},
                                             "gradient_clipping": 1.0})
    batch = long_batch(cfg, 8, 2048, 42)

    def step():
        out = eng(**batch)
        eng.backward(out["loss"])
        eng.step()
        return out
    ms, mn = timed(step, args.reps, warmup=2)
    out = step()
    torch.cuda.synchronize()
    res["lora_stage3_b8_s2048"] = {"ms_per_step": round(ms, 1), "min_ms": round(mn, 1), "loss": float(out["loss"].detach()),
                                   "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}
    print(res["lora_stage3_b8_s2048"], flush=True)
    del model, eng, lora, batch
    torch.cuda.empty_cache()

if "decode" not in skip:
    cfg = MedPLIBConfig.medplib_7b(moe_enable=True)
    model = MedPLIBForCausalLM(cfg, device=dev).eval()
    clip = torch.randn(1, 3, 336, 336, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16).to(dev)
    rows = []
    for S in (700, 8000):
        ids = long_batch(cfg, 1, S, 7)["input_ids"]
        t = {}
        for n_new in (16, 64):
            best = float("inf")
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model._greedy(ids, clip, n_new, -1)
                torch.cuda.synchronize()
                best = min(best, time.perf_counter() - t0)
            t[n_new] = best
        assert model.last_decode_path == "graph"
        rows.append({"prompt_positions": S, "ms_per_token": round((t[64] - t[16]) / 48 * 1e3, 3)})   # slope: prefill and capture cancel
        print(rows[-1], flush=True)
    res["decode_graph_7b_moe_e2"] = rows

print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
