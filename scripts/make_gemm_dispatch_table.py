"""Writes tests/golden/gemm_dispatch_table.json: which tile kernel (128 / 256 / 320) every bf16 GEMM call of the product, plus the
hand-written calls of tests/gemm_dispatch_cases.py, is dispatched to on an MI355X.  Run it on the commit whose selection is the reference;
tests/test_gpu_gemm_dispatch_table.py replays the table on every later one.

The product's calls are recorded by wrapping the GEMM wrappers of medplib_amd.ops (as scripts/gemm_census.py does for ops.gemm) around one
MoE training step at 7B dimensions (2 layers, B = 8; its CLIP and SAM towers run on their side streams), the two towers alone, one LoRA step
of the dense decoder and one evaluate() (prefill + a few decode steps).  Every distinct call is then issued again from its description
(zeros, no device-side rows); a call whose replay lands on another tile than the product's did is reported and left out.

    python scripts/make_gemm_dispatch_table.py [OUT.json]
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import bench
import gemm_dispatch_cases as cases
from medplib_amd import engine, ops
from medplib_amd.model.config import MedPLIBConfig
from medplib_amd.model.medplib import LISAForCausalLM, MedPLIBForCausalLM

dev = torch.device("cuda:0")
seen = {}            # key -> (row, tile the product's call got)


def note(entry, M, N, K, **kw):
    kw.setdefault("policy", ops._TILE_POLICY)
    kw.setdefault("stream", "side" if torch.cuda.current_stream().cuda_stream in ops._STREAM_WS else "primary")
    r = cases.row(entry, int(M), int(N), int(K), **kw)
    seen.setdefault(cases.key(r), (r, ops.gemm_last_kernel()))


real = {n: getattr(ops, n) for n in ("gemm", "gemm_swiglu_keep", "gemm_batched", "gemm_batched_res", "gemm_qkv_rope", "gemm_batched_rows")}


def gemm(a, w, bias=None, residual=None, act=ops.ACT_NONE, out_dtype=torch.bfloat16, out=None, alpha=1.0, m_dev=None):
    o = real["gemm"](a, w, bias=bias, residual=residual, act=act, out_dtype=out_dtype, out=out, alpha=alpha, m_dev=m_dev)
    note("mp_gemm_bf16_nt", a.shape[0], w.shape[0], a.shape[1], act=int(act), bias=bias is not None, residual=residual is not None,
         out="f32" if o.dtype == torch.float32 else "bf16", alpha=float(alpha), m_dev=m_dev is not None, lda=a.stride(0), ldc=o.stride(0))
    return o


def gemm_swiglu_keep(a, w, act_out=None):
    o = real["gemm_swiglu_keep"](a, w, act_out=act_out)
    note("mp_gemm_swiglu_keep_bf16", a.shape[0], w.shape[0], a.shape[1], act=5, lda=a.stride(0), ldc=o[0].stride(0))
    return o


def gemm_batched(a, w, out, m_dev=None, bias=None, act=ops.ACT_NONE):
    o = real["gemm_batched"](a, w, out, m_dev=m_dev, bias=bias, act=act)
    note("mp_gemm_bf16_nt_batched", a.shape[1], w.shape[1], a.shape[2], batch=a.shape[0], act=int(act), bias=bias is not None,
         out="f32" if out.dtype == torch.float32 else "bf16", m_dev=m_dev is not None)
    return o


def gemm_batched_res(a, w, residual, out, m_dev=None):
    o = real["gemm_batched_res"](a, w, residual, out, m_dev=m_dev)
    note("mp_gemm_bf16_nt_batched_res", a.shape[1], w.shape[1], a.shape[2], batch=a.shape[0], residual=True, m_dev=m_dev is not None)
    return o


def gemm_qkv_rope(a, w_interleaved, cos_t, sin_t, seq, heads, head_dim, pos_offset=0, out=None, row_scale=None):
    o = real["gemm_qkv_rope"](a, w_interleaved, cos_t, sin_t, seq, heads, head_dim, pos_offset=pos_offset, out=out, row_scale=row_scale)
    note("mp_gemm_qkv_rope_scaled_bounded_bf16" if row_scale is not None else "mp_gemm_qkv_rope_bounded_bf16", a.shape[0], w_interleaved.shape[0],
         a.shape[1], act=6, seq=int(seq), pos=int(pos_offset), lda=a.stride(0), ldc=o.stride(0))
    return o


def gemm_batched_rows(a, w, out, m_dev, a_rows=None, c_rows=None, c_scale=None, residual=None, act=ops.ACT_NONE, rows_stride=0, a_row_scale=None):
    o = real["gemm_batched_rows"](a, w, out, m_dev, a_rows=a_rows, c_rows=c_rows, c_scale=c_scale, residual=residual, act=act,
                                  rows_stride=rows_stride, a_row_scale=a_row_scale)
    E, N, K = w.shape
    note("mp_gemm_bf16_nt_batched_rows_scaled" if a_row_scale is not None else "mp_gemm_bf16_nt_batched_rows",
         rows_stride if a_rows is not None else a.shape[1], N, K, batch=E, act=int(act), residual=residual is not None, m_dev=m_dev is not None,
         a_rows=a_rows is not None, c_rows=c_rows is not None, lda=a.stride(0) if a_rows is not None else K,
         ldc=out.stride(0) if c_rows is not None else None)
    return o


for n in real:
    setattr(ops, n, globals()[n])


def attempt(what, fn):
    """The parts beside the two training steps only widen the table: one that fails is reported, not fatal."""
    try:
        fn()
    except Exception as e:
        print(f"[not recorded] {what}: {type(e).__name__}: {e}")


ds = {"train_micro_batch_size_per_gpu": 8, "optimizer": {"params": {"lr": 1e-4}}}
# one MoE training step (the towers on their side streams), then each tower alone on the calling stream
cfg = MedPLIBConfig.medplib_7b(num_hidden_layers=2)
model = MedPLIBForCausalLM(cfg, device=dev).train()
eng, _, _, _ = engine.initialize(model=model, model_parameters=model.trainable_parameters(), config=ds)
batch = bench.synthetic_batch(cfg, 8, dev, 42)
out = eng(**batch); eng.backward(out); eng.step()
model.sync_side_streams(); torch.cuda.synchronize()
vb = bench.vqa_batch(cfg, 1, dev, 0)
with torch.no_grad():
    model.eval()
    attempt("CLIP tower alone", lambda: model.get_model().vision_tower.encode_images(batch["images_clip"]))
    attempt("SAM encoder alone", lambda: model.get_visual_embs(batch["images"]))
    attempt("MoE evaluate()", lambda: model.evaluate(vb["images_clip"], vb["images"], vb["input_ids"], [(256, 256)], [(336, 336)], max_new_tokens=4,
                                                     eos_token_id=-1))
model.sync_side_streams(); torch.cuda.synchronize()
del eng, model, out
torch.cuda.empty_cache()
# the dense decoder's evaluate(), then one LoRA step (bench.lora_secondary's configuration)
cfg = MedPLIBConfig.medplib_7b(num_hidden_layers=2, moe_enable=False)
model = LISAForCausalLM(cfg, device=dev)
with torch.no_grad():               # (evaluate() works on the plain weights: before the adapters exist)
    model.eval()
    attempt("dense evaluate()", lambda: model.evaluate(vb["images_clip"], vb["images"], vb["input_ids"], [(256, 256)], [(336, 336)], max_new_tokens=4,
                                                       eos_token_id=-1))
model.train()
lora = model.enable_lora(lora_r=8, lora_alpha=16, lora_dropout=0.05, lora_target_modules="gate_proj,up_proj,down_proj",
                         sft_modules="mask_decoder,text_hidden_fcs")
eng, _, _, _ = engine.initialize(model=model, model_parameters=model.trainable_parameters(), config=ds)
out = eng(**batch); eng.backward(out); eng.step()
model.sync_side_streams(); torch.cuda.synchronize()
del eng, model, out, lora
torch.cuda.empty_cache()

for n in real:
    setattr(ops, n, real[n])
table, dropped = [], 0
for r, product_tile in list(seen.values()) + [(r, None) for r in cases.hand_rows() if cases.key(r) not in seen]:
    tile = cases.replay(r, dev)
    if product_tile is not None and tile != product_tile:
        print(f"[left out] the product's call got {product_tile}, its replay {tile}: {r}")
        dropped += 1
        continue
    table.append(dict(r, tile=tile, source="product" if product_tile is not None else "hand"))
entries, tiles = {r["entry"] for r in table}, {r["tile"] for r in table}
print(f"{len(table)} rows ({sum(r['source'] == 'product' for r in table)} from the product, {dropped} left out); entries {sorted(entries)}; tiles {sorted(tiles)}")
assert len(entries) == 10 and tiles == {128, 256, 320}, "the table must hold every entry point and every tile"
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "gemm_dispatch_table.json")
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, "w") as f:
    f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in table) + "\n]\n")
