"""Long sequences on the device: attention at S = 2048 .. 8192, the model past max_position_embeddings (prefill, LoRA training, decode across
the RoPE table's old edge), and the bounded RoPE / KV-append entry points (same bits as the unbounded ones in range; out of range they write
nothing and set the cache's error word)."""
import os

import numpy as np
import pytest
import torch

from medplib_amd import ops
from medplib_amd._lib import MedplibError, lib
from medplib_amd.model.config import MedPLIBConfig
from oracle import model as OM
from oracle import ops as O

pytestmark = pytest.mark.gpu

BF16_EPS = 2.0 ** -8


def _report(name, got, ref, rtol, atol):
    got, ref = got.float().cpu(), ref.float().cpu()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    print(f"{name}: max|err|={err.max().item():.4e}, ref absmax={ref.abs().max().item():.4e}, bad={int(bad.sum())}/{bad.numel()}")
    assert not bad.any(), name


# ------------------------------------------------------------------------------------------------ attention at long S
@pytest.mark.parametrize("S,ragged", [(2048, False), (4096, True), (8192, False)])
def test_attention_forward_long(dev, S, ragged):
    """Causal attention forward, head_dim 128, against fp32 torch computed one head at a time (test_attention's tolerance)."""
    B, H, D = 1, 2, 128
    g = torch.Generator().manual_seed(S)
    qkv = torch.randn(B, S, 3, H, D, generator=g).to(torch.bfloat16)
    kv = None
    if ragged:
        kv = torch.arange(S)[None, :] < S - 37
    dq = qkv.to(dev)
    out = ops.attention(dq[:, :, 0], dq[:, :, 1], dq[:, :, 2], causal=True, key_valid=None if kv is None else kv.to(torch.uint8).to(dev))
    torch.cuda.synchronize()
    out = out.float().cpu().view(B, S, H, D)
    mask = torch.tril(torch.ones(S, S, dtype=torch.bool))
    if kv is not None:
        mask &= kv[0][None, :]
    for h in range(H):
        q, k, v = (qkv[0, :, i, h].float() for i in range(3))
        p = torch.softmax((q @ k.t() * D ** -0.5).masked_fill(~mask, float("-inf")), -1)
        _report(f"attention S={S} head {h}", out[0, :, h], p @ v, rtol=3 * BF16_EPS, atol=2e-2)


def test_attention_backward_at_4096(dev):
    """Attention backward (fused delta) at S = 4096 against fp32 autograd (test_attention_backward_vs_autograd's bound: 2 % of each
    gradient's largest entry)."""
    B, H, S, D = 1, 2, 4096, 128
    g = torch.Generator().manual_seed(4096)
    qkv = (torch.randn(B, S, 3, H, D, generator=g) * 0.8).to(torch.bfloat16)
    d_out = torch.randn(B, S, H * D, generator=g).to(torch.bfloat16)
    q, k, v = [qkv[:, :, i].float().clone().requires_grad_(True) for i in range(3)]
    sc = torch.einsum("bqhd,bkhd->bhqk", q, k) * D ** -0.5
    sc = sc.masked_fill(~torch.tril(torch.ones(S, S, dtype=torch.bool))[None, None], float("-inf"))
    ref = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(sc, -1), v).reshape(B, S, H * D)
    ref.backward(d_out.float())
    qd = qkv.to(dev)
    out, lse2 = ops.attention_fwd_lse(qd[:, :, 0], qd[:, :, 1], qd[:, :, 2], causal=True)
    dq, dk, dv, _ = ops.attention_bwd(qd[:, :, 0], qd[:, :, 1], qd[:, :, 2], out, d_out.to(dev), lse2, causal=True)
    torch.cuda.synchronize()
    for name, got, want in (("dq", dq, q.grad), ("dk", dk, k.grad), ("dv", dv, v.grad)):
        err = (got.float().cpu() - want).abs().max().item()
        print(f"attention bwd S={S} {name}: max|err| {err:.3e}, ref absmax {want.abs().max().item():.3e}")
        assert err <= 2e-2 * want.abs().max().item() + 1e-3, name


# ------------------------------------------------------------------------------------------------ the model past 4096 positions
@pytest.mark.parametrize("prompt_len", [1725, 4125])
def test_full_size_parity_long_prompts(dev, prompt_len):
    """full_size_parity (2 MoE layers at the 7B dims, V = 4096) with S = prompt_len + 575: about 2300, and about 4700, which is past
    max_position_embeddings = 4096 (the RoPE tables grow).  The bounds of scripts/seq_len_parity.py."""
    from oracle.parity import full_size_parity
    cfg = MedPLIBConfig.medplib_7b(num_hidden_layers=2, vocab_size=4096, seg_token_idx=4000, moe_enable=True)
    torch.set_num_threads(min(16, os.cpu_count()))
    r = full_size_parity(cfg, dev, prompt_len=prompt_len)
    print({k: (round(v, 6) if isinstance(v, float) else v) for k, v in r.items() if k not in ("mask", "routing")})
    assert r["seq_len"] > prompt_len + 500 and (prompt_len < 4096 or r["seq_len"] > 4096)
    assert r["max_abs_dloss_over_10"] < 5e-2 and r["hidden_mean_rel_err"] < 2 ** -6 and r["routing_agreement_min"] >= 0.97, r


def _long_batch(cfg, L, seed):
    b = OM.make_batch(cfg, 1, L=L, H=96, Wd=80, seed=seed)
    b["images"] = b["images"].to(torch.bfloat16).float()
    b["images_clip"] = b["images_clip"].to(torch.bfloat16).float()
    return b


def test_lora_training_past_4096_positions(dev):
    """A LoRA step (adapters on q / v and gate / up / down, r = 8, dropout 0) at reduced width (hidden 1024, 8 heads x 128, 2 dense layers)
    with S = 4374 > max_position_embeddings: the forward grows cos / sin, the backward's transposed RoPE reads the grown sin_neg.  Every
    adapter gradient against the oracle's fp32 autograd, with test_lora_gradients_at_true_dims' bounds."""
    from medplib_amd import engine
    from medplib_amd.model.medplib import LISAForCausalLM
    torch.set_num_threads(min(16, os.cpu_count()))
    cfg = MedPLIBConfig.medplib_7b(hidden_size=1024, intermediate_size=2816, num_attention_heads=8, num_hidden_layers=2, vocab_size=4096,
                                   seg_token_idx=4000, moe_enable=False, moe_gate_sampling=False)
    W = OM.init_hf_weights_aliased(cfg, seed=0)
    m = LISAForCausalLM(cfg, device=dev).train()
    m.load_hf_state_dict(W)
    r, alpha = 8, 16
    lora = m.enable_lora(lora_r=r, lora_alpha=alpha, lora_dropout=0.0, lora_target_modules="q_proj,v_proj,gate_proj,up_proj,down_proj",
                         sft_modules="mask_decoder,text_hidden_fcs")
    g = torch.Generator().manual_seed(31)
    Wl = dict(W)
    Wl["lora_scaling"] = alpha / r
    for n, p_ in zip(lora.names, lora.params):
        if "lora_" in n:
            v = (torch.randn(p_.shape, generator=g) * (0.02 if "lora_A" in n else 0.01)).to(torch.bfloat16).float()
            p_.data.copy_(v.to(dev))
        else:
            v = p_.detach().float().cpu()
        Wl[n] = v.clone().requires_grad_(True)
    batch = _long_batch(cfg, 3800, seed=42)
    ref = OM.model_forward(batch, Wl, cfg, training=True, llm_grad=True)
    ref["loss"].backward()
    eng, _, _, _ = engine.initialize(model=m, model_parameters=m.trainable_parameters(),
                                     config={"optimizer": {"params": {"lr": 1e-4, "betas": (0.9, 0.95)}}, "gradient_clipping": 1.0})
    gb = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
    gb["masks_list"] = [x.to(dev) for x in batch["masks_list"]]
    out = eng(**gb)
    eng.backward(out["loss"])
    torch.cuda.synchronize()
    llm = m.model.llm
    assert llm.cos.shape[0] == 5120 and llm.sin_neg.shape[0] == 5120 and torch.equal(llm.sin_neg, -llm.sin)
    worst, adapters = 0.0, 0
    for n, p_ in zip(lora.names, lora.params):
        if "lora_" not in n:
            continue
        want = Wl[n].grad
        rel = (p_.grad.float().cpu() - want).abs().max().item() / (want.abs().max().item() + 1e-30)
        worst, adapters = max(worst, rel), adapters + 1
    dloss = max(abs(float(out[k].detach()) - float(ref[k])) for k in O.LOSS_KEYS)
    print(f"LoRA S=4374: {adapters} adapter tensors, worst rel {worst:.4f}, max |dloss| {dloss:.3e}")
    assert adapters == 2 * 2 * 5 and worst < 0.05 and dloss < 2e-2


def test_forward_bits_unchanged_by_a_grown_table(dev):
    """An existing-length forward (S = 639, hidden 1024, 2 MoE layers) gives the same bits before and after the tables grew to 9216 rows."""
    from medplib_amd.model.llama import LlamaStack
    cfg = MedPLIBConfig.medplib_7b(hidden_size=1024, intermediate_size=2816, num_attention_heads=8, num_hidden_layers=2, vocab_size=4096,
                                   moe_enable=True, moe_gate_sampling=False)
    st = LlamaStack(cfg, dev, seed=5)
    st.training = False
    emb = (torch.randn(1, 639, 1024, generator=torch.Generator().manual_seed(3)) * 0.5).to(torch.bfloat16).to(dev)
    a = st.forward(emb, None)[0].clone()
    st.ensure_positions(9000)
    assert st.cos.shape[0] == 9216
    b = st.forward(emb, None)[0]
    torch.cuda.synchronize()
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ decode across the table edge
def _greedy(m, batch, n_new, graph):
    m.decode_with_graph = graph
    clip = batch["images_clip"].to(torch.bfloat16).to(m.device_)
    ids, hid = m._greedy(np.asarray(batch["input_ids"]).astype(np.int64), clip, n_new, -1)
    torch.cuda.synchronize()
    return ids, [h.clone() for h in hid]


@pytest.mark.parametrize("S", [4090, 8180])
def test_decode_across_the_table_edge(dev, S):
    """Prompt of S positions + 24 new tokens at reduced width (hidden 512, 4 heads x 128, 2 top-1 MoE layers, max_position_embeddings 4096):
    the fed tokens sit at positions S .. S + 22, across 4096 (and across 8192 after new_kv_cache grew the table to 9216 rows).  The graph and
    the token-by-token loop give equal ids and hidden states (bit-equal but for single roundings, see below); the ids equal the oracle's cache-free greedy decode (a divergence only
    at a step whose oracle top-2 logit gap is below 0.05, the rule of the other decode tests)."""
    from medplib_amd.model.medplib import MedPLIBForCausalLM
    torch.set_num_threads(min(16, os.cpu_count()))
    cfg = MedPLIBConfig.tiny(moe_enable=True, sam_depth=2, hidden_size=512, num_attention_heads=4, intermediate_size=640)
    assert cfg.max_position_embeddings == 4096
    W = OM.init_hf_weights(cfg, seed=3)
    m = MedPLIBForCausalLM(cfg, device=dev).eval()
    m.load_hf_state_dict(W)
    n_img = (cfg.clip_image_size // cfg.clip_patch_size) ** 2
    batch = OM.make_batch(cfg, 1, L=S - n_img + 1, seed=0)
    n_new = 24
    ids_g, hid_g = _greedy(m, batch, n_new, True)
    assert m.last_decode_path == "graph"
    assert hid_g[0].shape[1] == S and m.model.llm.cos.shape[0] >= S + n_new
    ids_l, hid_l = _greedy(m, batch, n_new, False)
    assert m.last_decode_path == "loop"
    assert np.array_equal(ids_g, ids_l) and ids_g.shape[1] == batch["input_ids"].shape[1] + n_new
    assert len(hid_g) == len(hid_l) == n_new
    # the prompt's hidden state is bit-equal; a fed token's may differ in one bf16 rounding between the two paths, at single steps, at any
    # long length (measured: one step of 24 at S = 2000, below every table edge, as at S = 4090; none at 8180) — a property of the two
    # paths' decode kernels that this change does not touch
    assert torch.equal(hid_g[0], hid_l[0])
    differing = [i for i, (a, b) in enumerate(zip(hid_g, hid_l)) if not torch.equal(a, b)]
    for i in differing:
        a, b = hid_g[i].float(), hid_l[i].float()
        assert float((a - b).abs().max()) <= 2 ** -6 * float(b.abs().max()), i
    print(f"S={S}: graph vs loop hidden states differ (<= 1 bf16 rounding) at steps {differing}")
    assert len(differing) <= 2, differing
    bq = dict(batch, images_clip=batch["images_clip"].to(torch.bfloat16).float(), images=batch["images"].to(torch.bfloat16).float())
    ids_ref, _, dbg = OM.evaluate(bq, W, cfg, max_new_tokens=n_new, eos_token_id=-1, return_debug=True)
    a, b = ids_g[0].tolist(), ids_ref[0].tolist()
    n_in = batch["input_ids"].shape[1]
    agree = 0
    while agree < min(len(a), len(b)) and a[agree] == b[agree]:
        agree += 1
    print(f"S={S}: generated {a[n_in:]} vs oracle {b[n_in:]}")
    if agree < max(len(a), len(b)):
        step = agree - n_in
        assert 0 <= step < len(dbg["gaps"]) and dbg["gaps"][step] < 5e-2, "token ids diverge from the oracle at a step that is not a near tie"


# ------------------------------------------------------------------------------------------------ bounded entry points
def _decode_case(g, B, H, D, K, rows, dev):
    d = H * D
    x = torch.randn(B, K, generator=g).to(torch.bfloat16).to(dev)
    w = (torch.randn(3 * d, K, generator=g) * 0.05).to(torch.bfloat16).to(dev)
    nw = (1.0 + 0.2 * torch.randn(K, generator=g)).to(dev)
    ang = torch.rand(rows, D // 2, generator=g) * 6.28
    cos_t, sin_t = ang.cos().contiguous().to(dev), ang.sin().contiguous().to(dev)
    fill = torch.randn(B, rows, H, D, generator=g).to(torch.bfloat16).to(dev)
    return x, w, nw, cos_t, sin_t, fill


def _old_decode_rope_append(qkv, cos_t, sin_t, ck, cv, posd, H, D):
    lib().call("mp_decode_rope_append_bf16", qkv.data_ptr(), qkv.stride(0), cos_t.data_ptr(), sin_t.data_ptr(), ck.data_ptr(), cv.data_ptr(),
               posd.data_ptr(), qkv.shape[0], H, D, ck.stride(0), ck.stride(1), torch.cuda.current_stream().cuda_stream)


def _old_gemv_rope_append(x, nw, w, cos_t, sin_t, ck, cv, posd, H, D):
    qkv = torch.empty((x.shape[0], 3 * H * D), dtype=torch.bfloat16, device=x.device)
    lib().call("mp_gemv_rmsnorm_rope_append_bf16", x.data_ptr(), x.stride(0), nw.data_ptr(), 1e-5, w.data_ptr(), w.stride(0), qkv.data_ptr(),
               qkv.stride(0), cos_t.data_ptr(), sin_t.data_ptr(), ck.data_ptr(), cv.data_ptr(), posd.data_ptr(), x.shape[0], H, D, x.shape[1],
               ck.stride(0), ck.stride(1), torch.cuda.current_stream().cuda_stream)
    return qkv


def test_bounded_decode_kernels_equal_the_unbounded_ones(dev):
    """In range, mp_decode_rope_append_bounded_bf16 and mp_gemv_rmsnorm_rope_append_bounded_bf16 (what ops routes to) write the bits of
    the unbounded entry points, at the first and last rows of the table and the cache, and leave the error word at 0."""
    g = torch.Generator().manual_seed(41)
    for (B, H, D, K, rows) in [(1, 32, 128, 4096, 700), (2, 4, 64, 512, 300), (2, 8, 128, 1024, 129)]:
        x, w, nw, cos_t, sin_t, fill = _decode_case(g, B, H, D, K, rows, dev)
        for pos in (0, rows // 2, rows - 1):
            posd = torch.tensor([pos], dtype=torch.int32, device=dev)
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            base = ops.gemv(ops.rmsnorm(x, nw, 1e-5), w)
            ref, got = base.clone(), base.clone()
            ck_a, cv_a, ck_b, cv_b = fill.clone(), fill.clone(), fill.clone(), fill.clone()
            _old_decode_rope_append(ref, cos_t, sin_t, ck_a, cv_a, posd, H, D)
            ops.decode_rope_append(got, cos_t, sin_t, ck_b, cv_b, posd, H, D, err=err)
            torch.cuda.synchronize()
            assert torch.equal(got, ref) and torch.equal(ck_b, ck_a) and torch.equal(cv_b, cv_a), (B, H, D, pos)
            assert not torch.equal(ck_b[:, pos], fill[:, pos])
            if K % 512 == 0 and B <= 2:
                ck_a, cv_a, ck_b, cv_b = fill.clone(), fill.clone(), fill.clone(), fill.clone()
                q_old = _old_gemv_rope_append(x, nw, w, cos_t, sin_t, ck_a, cv_a, posd, H, D)
                q_new = ops.gemv_rmsnorm_rope_append(x, nw, 1e-5, w, cos_t, sin_t, ck_b, cv_b, posd, H, D, err=err)
                torch.cuda.synchronize()
                d = H * D
                assert torch.equal(q_new[:, :d], q_old[:, :d]) and torch.equal(ck_b, ck_a) and torch.equal(cv_b, cv_a), (B, H, D, pos, "gemv")
            assert int(err[0]) == 0


def test_bounded_decode_kernels_write_nothing_past_a_bound(dev):
    """A position inside the real tables and caches but at or past the bound the call is given (a shorter view of the table, of the cache)
    writes neither q nor a cache row and sets MP_POS_ERR_TABLE (1) / MP_POS_ERR_CACHE (2) in the error word, sticky across calls.  No
    memory outside the real allocations is touched."""
    g = torch.Generator().manual_seed(43)
    B, H, D, K, rows = 1, 8, 128, 1024, 700
    x, w, nw, cos_t, sin_t, fill = _decode_case(g, B, H, D, K, rows, dev)
    pos = 500
    posd = torch.tensor([pos], dtype=torch.int32, device=dev)
    for fused in (False, True):
        for t_rows, c_rows, code in ((300, rows, 1), (rows, 400, 2), (pos, pos, 3), (pos + 1, pos + 1, 0)):
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            ck, cv = fill.clone(), fill.clone()
            qkv = ops.gemv(ops.rmsnorm(x, nw, 1e-5), w)
            before = qkv.clone()
            if fused:       # (its q output buffer: test_fused_gemv_leaves_q_unwritten_past_a_bound)
                ops.gemv_rmsnorm_rope_append(x, nw, 1e-5, w, cos_t[:t_rows], sin_t[:t_rows], ck[:, :c_rows], cv[:, :c_rows], posd, H, D, err=err)
            else:
                ops.decode_rope_append(qkv, cos_t[:t_rows], sin_t[:t_rows], ck[:, :c_rows], cv[:, :c_rows], posd, H, D, err=err)
            torch.cuda.synchronize()
            assert int(err[0]) == code, (fused, t_rows, c_rows, int(err[0]))
            if code:
                assert torch.equal(ck, fill) and torch.equal(cv, fill), (fused, t_rows, c_rows)
                assert fused or torch.equal(qkv, before)
            else:
                assert not torch.equal(ck[:, pos], fill[:, pos])
        # sticky: a later in-range call leaves the bit set
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        ops.decode_rope_append(ops.gemv(ops.rmsnorm(x, nw, 1e-5), w), cos_t[:300], sin_t[:300], fill.clone(), fill.clone(), posd, H, D, err=err)
        ops.decode_rope_append(ops.gemv(ops.rmsnorm(x, nw, 1e-5), w), cos_t, sin_t, fill.clone(), fill.clone(), posd, H, D, err=err)
        torch.cuda.synchronize()
        assert int(err[0]) == 1


def test_fused_gemv_leaves_q_unwritten_past_a_bound(dev):
    """mp_gemv_rmsnorm_rope_append_bounded_bf16 past the table: the q third of its output buffer is not written (the buffer keeps a marker)."""
    g = torch.Generator().manual_seed(47)
    B, H, D, K, rows = 1, 8, 128, 1024, 700
    x, w, nw, cos_t, sin_t, fill = _decode_case(g, B, H, D, K, rows, dev)
    posd = torch.tensor([600], dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    qkv = torch.full((B, 3 * H * D), 7.0, dtype=torch.bfloat16, device=dev)
    ck, cv = fill.clone(), fill.clone()
    lib().call("mp_gemv_rmsnorm_rope_append_bounded_bf16", x.data_ptr(), x.stride(0), nw.data_ptr(), 1e-5, w.data_ptr(), w.stride(0),
               qkv.data_ptr(), qkv.stride(0), cos_t.data_ptr(), sin_t.data_ptr(), ck.data_ptr(), cv.data_ptr(), posd.data_ptr(), B, H, D, K,
               ck.stride(0), ck.stride(1), 600, rows, err.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert int(err[0]) == 1 and bool((qkv == 7.0).all()) and torch.equal(ck, fill) and torch.equal(cv, fill)


def test_prefill_rope_past_the_table_raises(dev):
    """ops.rope_qk_ / ops.gemm_qkv_rope with a table shorter than seq + pos_offset raise MedplibError (no assert, no launch)."""
    H, D, S = 2, 128, 64
    ang = torch.rand(100, D // 2) * 6.28
    cos_t, sin_t = ang.cos().contiguous().to(dev), ang.sin().contiguous().to(dev)
    qkv = torch.randn(S, 3 * H * D).to(torch.bfloat16).to(dev)
    before = qkv.clone()
    with pytest.raises(MedplibError, match="table_rows = 100"):
        ops.rope_qk_(qkv, cos_t, sin_t, S, H, D, pos_offset=37)
    ops.rope_qk_(qkv, cos_t, sin_t, S, H, D, pos_offset=36)            # 36 + 64 = 100 rows: fits
    torch.cuda.synchronize()
    assert not torch.equal(qkv, before)
    d = 256
    a = torch.randn(S, d).to(torch.bfloat16).to(dev)
    wi = ops.rope_interleave_qkv((torch.randn(3 * d, d) * 0.05).to(torch.bfloat16).to(dev), H, D)
    with pytest.raises(MedplibError, match="table_rows = 100"):
        ops.gemm_qkv_rope(a, wi, cos_t, sin_t, S, H, D, pos_offset=40)
