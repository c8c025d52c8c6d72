"""Top-2 MoE decode on the device: the one-launch norm + gate + top-2 routing, the two-expert GEMVs, the decode step that uses them, and the
captured decode graph of evaluate() / generate() for top-2 models (plain and with the gate's Gumbel sampling, whose draws the graph keys on
a device-side pass counter).  Every comparison is bit for bit unless stated otherwise."""
import numpy as np
import pytest
import torch

from medplib_amd import ops
from medplib_amd.model.config import MedPLIBConfig
from oracle import model as OM

pytestmark = pytest.mark.gpu


def _model(cfg, dev, W):
    from medplib_amd.model.medplib import MedPLIBForCausalLM
    m = MedPLIBForCausalLM(cfg, device=dev)
    m.load_hf_state_dict(W)
    return m


# ------------------------------------------------------------------------------------------------ routing kernel
def test_fused_top2_route_equals_separate_kernels(dev):
    """mp_decode_norm_gate_route_top2 vs mp_rmsnorm_bf16 + mp_moe_gate_bf16 + mp_moe_route_top2 over T in {1, 2, 5, 8}, E in {2, 3, 4, 8},
    a capacity that binds and one that does not, injected exact logit ties (equal gate rows, equal draws), with and without Gumbel draws:
    the normed rows, expert / slot / weight of both choices, kept, counts and l_aux."""
    g = torch.Generator().manual_seed(5)
    dropped = ties_on_top = 0
    for d in (4096, 256):
        for T in (1, 2, 5, 8):
            for E in (2, 3, 4, 8):
                for cap in (1, 2 * T):
                    for tie in (False, True):
                        for with_noise in (False, True):
                            x = (torch.randn(T, d, generator=g) * 2).to(torch.bfloat16)
                            ln_w = 1 + 0.1 * torch.randn(d, generator=g)
                            wg = torch.randn(E, d, generator=g) * 0.05
                            noise = -torch.log(-torch.log(torch.rand(T, E, generator=g).clamp_(1e-6, 1 - 1e-6))) if with_noise else None
                            if tie:                       # experts 0 / 1 (and 2 / 3) have identical logits and identical draws
                                wg[1] = wg[0]
                                if E >= 4:
                                    wg[3] = wg[2]
                                if noise is not None:
                                    noise[:, 1] = noise[:, 0]
                                    if E >= 4:
                                        noise[:, 3] = noise[:, 2]
                            x, ln_w, wg = x.to(dev), ln_w.to(dev), wg.to(dev)
                            noise = None if noise is None else noise.to(dev)
                            h_ref = ops.rmsnorm(x, ln_w, 1e-5)
                            logits, gates = ops.moe_gate(h_ref, wg)
                            ref = ops.moe_route_top2(gates, logits, cap, noise)
                            got = ops.decode_norm_gate_route_top2(x, ln_w, 1e-5, wg, cap, noise)
                            torch.cuda.synchronize()
                            case = (d, T, E, cap, tie, with_noise)
                            assert torch.equal(got[0], h_ref), case
                            for a, b, name in zip(got[1:], ref, ["expert", "slot", "weight", "kept", "counts", "l_aux"]):
                                assert torch.equal(a, b), (name, case, a, b)
                            dropped += int((got[2] < 0).sum())
                            if tie:
                                ex = got[1].cpu()
                                ties_on_top += int(((ex[:T] == 0) & (ex[T:] == 1)).sum())
    assert dropped > 0, "the binding capacity dropped nothing"
    assert ties_on_top > 0, "no tied pair of experts was ever the top two"


# ------------------------------------------------------------------------------------------------ expert GEMVs
def _route_with_drops(T, E, cap, dev, g):
    """Routing of T decode rows with a known pattern: first choices alternate between experts 0 and 1, every second choice is expert 2,
    so with capacity 3 the rows 3.. lose their second choice and rows 6, 7 both choices."""
    logits = torch.randn(T, E, generator=g) * 0.1
    for t in range(T):
        logits[t, t % 2] += 5.0
        logits[t, 2] += 2.0
    logits = logits.to(dev)
    gates = torch.softmax(logits, dim=1)
    return ops.moe_route_top2(gates, logits, cap)


@pytest.mark.parametrize("B", [1, 8])
def test_top2_expert_gemvs_equal_the_existing_kernels(dev, B):
    """At d = 4096, ff = 11008, E = 3: mp_gemv_top2_gate_up_bf16 + mp_gemv_top2_down_bf16 equal, bit for bit, the composition of the kernels
    the top-1 decode already uses — per (token, choice) entry the expert-indexed SwiGLU GEMV and the expert-indexed down GEMV — followed by
    mp_moe_combine_bf16 (first choice, then second, then the residual).  B = 8 with capacity 3 drops second choices (rows 3-7) and both
    choices (rows 6, 7).  Against the batched expert GEMMs (MFMA tiles: another fp32 summation order) the result agrees to bf16 rounding."""
    d, ff, E = 4096, 11008, 3
    g = torch.Generator().manual_seed(40 + B)
    gu = (torch.randn(E, 2 * ff, d, generator=g) * 0.02).to(torch.bfloat16).to(dev)
    down = (torch.randn(E, d, ff, generator=g) * 0.02).to(torch.bfloat16).to(dev)
    h = torch.randn(B, d, generator=g).to(torch.bfloat16).to(dev)
    x = torch.randn(B, d, generator=g).to(torch.bfloat16).to(dev)
    cap = 3 if B == 8 else 2
    expert, slot, weight, kept, _, _ = _route_with_drops(B, E, cap, dev, g)
    sl = slot.cpu()
    if B == 8:
        assert (sl[B:] < 0).any() and (sl[B:] >= 0).any() and (sl[:B] >= 0).any()
        assert ((sl[:B] >= 0) & (sl[B:] < 0)).any(), "no row with a kept first and a dropped second choice"
    act = ops.gemv_top2_gate_up(h, gu, expert, slot)
    out = ops.gemv_top2_down(act, down, expert, slot, weight, x)
    # the same entries through mp_gemv_bf16 (M = 1, w_index) and the combine kernel
    ybuf = torch.zeros((E, cap, d), dtype=torch.bfloat16, device=dev)
    for e in range(2 * B):
        if sl[e] < 0:
            continue
        a_e = ops.gemv(h[e % B:e % B + 1], gu, act=ops.ACT_SWIGLU_PAIR, w_index=expert[e:e + 1])
        assert torch.equal(act[e:e + 1], a_e), e
        ybuf[int(expert[e]), int(sl[e])] = ops.gemv(a_e, down, w_index=expert[e:e + 1])[0]
    ref = ops.moe_combine(ybuf, expert, slot, weight, x, cap, top_k=2)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    if B == 8:
        assert torch.equal(out[6:8], x[6:8].float().to(torch.bfloat16))           # both choices dropped: the residual stream (x + 0)
    # the batched-GEMM composition (the expert path of multi-row top-2 layers)
    buf = ops.moe_dispatch(h, expert, slot, E, cap, top_k=2)
    act_b = torch.empty((E, cap, ff), dtype=torch.bfloat16, device=dev)
    ops.gemm_batched(buf, gu, act_b, m_dev=kept, act=ops.ACT_SWIGLU_PAIR)
    y_b = torch.empty((E, cap, d), dtype=torch.bfloat16, device=dev)
    ops.gemm_batched(act_b, down, y_b, m_dev=kept)
    ref_b = ops.moe_combine(y_b, expert, slot, weight, x, cap, top_k=2)
    diff = (out.float() - ref_b.float()).abs().max().item()
    print(f"B={B}: fused two-expert GEMVs vs batched expert GEMMs: max |diff| {diff:.3e} (|out| max {out.float().abs().max().item():.2f})")
    assert diff <= 2 ** -6 * out.float().abs().max().item()


# ------------------------------------------------------------------------------------------------ decode step
def _stack_7b(dev, **kw):
    from medplib_amd.model.llama import LlamaStack
    cfg = MedPLIBConfig.medplib_7b(num_hidden_layers=2, vocab_size=1024, moe_enable=True, num_experts=3, top_k_experts=2, **kw)
    st = LlamaStack(cfg, dev, seed=3)
    st.training = False
    return st


def _decode_run(st, B, fuse, steps=6, S=5, device_pass=False, seed=17):
    g = torch.Generator().manual_seed(seed)
    d = st.cfg.hidden_size
    emb = (torch.randn(B, S + steps, d, generator=g) * 0.5).to(torch.bfloat16).to(st.device)
    st.fuse_decode_routing = fuse
    st.gate_pass, st._draws_key = 0, None
    cache = st.new_kv_cache(B, S + steps + 3)
    st.forward(emb[:, :S].contiguous(), None, kv_cache=cache)                      # prefill
    counters = torch.tensor([S, S + 1], dtype=torch.int32, device=st.device)
    pass_dev = torch.tensor([st.gate_pass + 1], dtype=torch.int32, device=st.device) if device_pass else None
    hs = []
    for k in range(steps):
        hs.append(st.decode_step(emb[:, S + k:S + k + 1].contiguous(), cache, counters, pass_dev=pass_dev).clone())
        ops.advance_ints(counters, 1)
        if pass_dev is not None:
            ops.advance_ints(pass_dev, 1)
    torch.cuda.synchronize()
    n = S + steps
    return hs, [c[:, :n].clone() for c in cache["k"]], [c[:, :n].clone() for c in cache["v"]]


@pytest.mark.parametrize("B", [1, 3])
def test_decode_step_top2_fused_equals_unfused(dev, B):
    """A 2-layer top-2 stack (E = 3) at the 7B layer dims, gate sampling on (Gumbel draws of the second choice): decode_step with the fused
    top-2 routing launch equals the separate rmsnorm / gate / route kernels of _mlp, in the hidden state of every step and in the KV-cache
    contents; the draws keyed on a device-side pass counter equal the host-keyed ones; and with injected draws (rts_uniform_provider)."""
    st = _stack_7b(dev)
    assert st.cfg.moe_gate_sampling
    ref = _decode_run(st, B, fuse=False)
    got = _decode_run(st, B, fuse=True)
    dev_keyed = _decode_run(st, B, fuse=True, device_pass=True)
    for run in (got, dev_keyed):
        for a, b in zip(run[0], ref[0]):
            assert torch.equal(a, b)
        for a, b in zip(run[1] + run[2], ref[1] + ref[2]):
            assert torch.equal(a, b)
    g = torch.Generator().manual_seed(9)
    draws = {}

    def provider(i, T, E_):
        if (i, T) not in draws:
            draws[(i, T)] = -torch.log(-torch.log(torch.rand(T, E_, generator=g).clamp_(1e-6, 1 - 1e-6))).to(dev)
        return draws[(i, T)]
    st.rts_uniform_provider = provider
    ref_p = _decode_run(st, B, fuse=False)
    got_p = _decode_run(st, B, fuse=True)
    assert all(torch.equal(a, b) for a, b in zip(got_p[0], ref_p[0]))
    assert all(torch.equal(a, b) for a, b in zip(got_p[1] + got_p[2], ref_p[1] + ref_p[2]))
    assert not all(torch.equal(a, b) for a, b in zip(got_p[0], ref[0])), "the injected draws changed nothing"


# ------------------------------------------------------------------------------------------------ end to end
def _tiny_top2(dev, **kw):
    cfg = MedPLIBConfig.tiny(moe_enable=True, sam_depth=2, num_experts=3, top_k_experts=2, **kw)
    W = OM.init_hf_weights(cfg, seed=3)
    return cfg, W, _model(cfg, dev, W).eval()


def _greedy(m, batch, n_new, eos, graph):
    m.decode_with_graph = graph
    clip = batch["images_clip"].to(torch.bfloat16).to(m.device_)
    ids, hid = m._greedy(np.asarray(batch["input_ids"]).astype(np.int64), clip, n_new, eos)
    torch.cuda.synchronize()
    return ids, [h.clone() for h in hid]


def test_top2_graph_decode_equals_the_loop_and_the_oracle(dev):
    """A tiny E = 3 top-2 model, 40 new tokens (three EOS-check windows of the graph loop): the captured-graph decode gives the token ids
    and the hidden state of every fed token of the token-by-token loop, for evaluate() (ids and mask) and generate(); last_decode_path says
    which path ran.  The greedy ids equal the CPU oracle's cache-free greedy decode of the same weights (a divergence is accepted only at a
    step whose oracle top-2 logit gap is below bf16 noise, as in the top-1 test)."""
    cfg, W, m = _tiny_top2(dev)
    batch = OM.make_batch(cfg, 1, seed=0)
    ids_g, hid_g = _greedy(m, batch, 40, -1, True)
    assert m.last_decode_path == "graph"
    ids_l, hid_l = _greedy(m, batch, 40, -1, False)
    assert m.last_decode_path == "loop"
    assert np.array_equal(ids_g, ids_l) and ids_g.shape[1] == batch["input_ids"].shape[1] + 40
    assert len(hid_g) == len(hid_l) == 40
    for a, b in zip(hid_g, hid_l):
        assert torch.equal(a, b)
    # evaluate(): ids and the mask of the picked row
    bq = dict(batch, images_clip=batch["images_clip"].to(torch.bfloat16).float(), images=batch["images"].to(torch.bfloat16).float())
    outs = {}
    for graph in (True, False):
        m.decode_with_graph = graph
        outs[graph] = m.evaluate(bq["images_clip"].to(dev), bq["images"].to(dev), bq["input_ids"], batch["resize_list"], batch["label_list"],
                                 max_new_tokens=40, eos_token_id=-1)
        assert m.last_decode_path == ("graph" if graph else "loop")
    assert torch.equal(outs[True][0], outs[False][0]) and torch.equal(outs[True][1][0], outs[False][1][0])
    # generate(): a 2-row padded batch
    b2 = OM.make_batch(cfg, 2, ragged=True, seed=4)
    clip2 = b2["images_clip"].to(dev).to(torch.bfloat16)
    m.decode_with_graph = True
    gen_g = m.generate(b2["input_ids"], images=clip2, attention_mask=b2["attention_mask"], max_new_tokens=40, eos_token_id=-1)
    assert m.last_decode_path == "graph"
    m.decode_with_graph = False
    gen_l = m.generate(b2["input_ids"], images=clip2, attention_mask=b2["attention_mask"], max_new_tokens=40, eos_token_id=-1)
    assert torch.equal(gen_g, gen_l)
    # the oracle
    ids_ref, _, dbg = OM.evaluate(bq, W, cfg, max_new_tokens=40, return_debug=True)
    a, b = outs[True][0][0].tolist(), ids_ref[0].tolist()
    n_in = bq["input_ids"].shape[1]
    agree = 0
    while agree < min(len(a), len(b)) and a[agree] == b[agree]:
        agree += 1
    print(f"generated {a[n_in:]} vs oracle {b[n_in:]}")
    if agree < max(len(a), len(b)):
        step = agree - n_in
        assert 0 <= step < len(dbg["gaps"]) and dbg["gaps"][step] < 5e-2, "token ids diverge from the oracle at a step that is not a near tie"


def test_top2_graph_decode_with_gate_sampling_equals_the_loop(dev):
    """moe_gate_sampling on (seeded Gumbel draws of the second choice, keyed on the forward-pass number): two evaluate() calls in a row
    through the graph give the ids of two calls through the loop — the second call also checks that the graph leaves the host pass counter
    where the loop leaves it, with an EOS inside the last check window (replays past it are discarded).  The draws do change the result."""
    cfg, W, m = _tiny_top2(dev, moe_gate_sampling=True, moe_gate_seed=7)
    batch = OM.make_batch(cfg, 1, seed=2)
    llm = m.model.llm
    start = llm.gate_pass
    probe, _ = _greedy(m, batch, 40, -1, False)
    n_in = batch["input_ids"].shape[1]
    eos = int(probe[0, n_in + 36])                      # a token late in the run: the graph replays past it in its last window
    eos = eos if eos not in probe[0, n_in:n_in + 36].tolist() else -1
    runs = {}
    for graph in (True, False):
        llm.gate_pass = start
        r1, h1 = _greedy(m, batch, 40, eos, graph)
        assert m.last_decode_path == ("graph" if graph else "loop")
        r2, h2 = _greedy(m, batch, 40, eos, graph)
        runs[graph] = (r1, h1, r2, h2, llm.gate_pass)
    g, l = runs[True], runs[False]
    assert np.array_equal(g[0], l[0]) and np.array_equal(g[2], l[2]) and g[4] == l[4]
    assert all(torch.equal(a, b) for a, b in zip(g[1] + g[3], l[1] + l[3]))
    assert not np.array_equal(g[0], g[2]) or not all(torch.equal(a, b) for a, b in zip(g[1], g[3])), \
        "two passes with different draws decoded identically: the sampling was not exercised"
    # the graph refuses injected host-side draws (they would be frozen into it) and takes the loop
    llm.rts_uniform_provider = lambda i, T, E: torch.zeros(T * E, dtype=torch.float32, device=dev)
    _greedy(m, batch, 8, -1, True)
    assert m.last_decode_path == "loop"
    llm.rts_uniform_provider = None
