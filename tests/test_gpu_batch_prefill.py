"""Batched prefill of a decode group (batch_prefill=True): the prompts right-padded through ONE LlamaStack.forward(seg_lens=), every MoE layer
routing each prompt as a pass of its own, on the tiny config (dense, E = 2 top-1, E = 2 top-2).  What is exact is tested exactly: a group of
one, the order of the batch-mates (also with a capacity that drops tokens), each layer's routing against the unsegmented op on the layer's
own gate input, graph against loop, the output layout.  A row against the single-prompt model is another summation order: the dense kind
under the bound tests/test_gpu_generate_batch.py holds the per-row path to; the MoE kinds are covered by the exact tests."""
import json

import numpy as np
import pytest
import torch

from medplib_amd import ops
from medplib_amd.model import generation as G
from medplib_amd.model.config import MedPLIBConfig
from oracle import model as OM

pytestmark = pytest.mark.gpu

KINDS = ("dense", "top1", "top2")
MOE = ("top1", "top2")
N_NEW = 16
BOUND = 2.0 ** -5            # "same function, another summation order" (BOUND of tests/test_gpu_generate_batch.py)
LENGTHS = (24, 31, 17)
EOS = 2
SEGMENTED = {"top1": "moe_route_top1_segments", "top2": "moe_route_top2_segments"}


def _tiny(dev, kind, **kw):
    from medplib_amd.model.medplib import LISAForCausalLM, MedPLIBForCausalLM
    if kind == "dense":
        cfg, cls = MedPLIBConfig.tiny(moe_enable=False, sam_depth=2, **kw), LISAForCausalLM
    else:
        cfg, cls = MedPLIBConfig.tiny(moe_enable=True, sam_depth=2, num_experts=2, top_k_experts=1 if kind == "top1" else 2, **kw), MedPLIBForCausalLM
    m = cls(cfg, device=dev)
    m.load_hf_state_dict(OM.init_hf_weights(cfg, seed=3))
    return cfg, m.eval()


def _prompts(cfg, dev, lengths=LENGTHS):
    """One (ids [1, L], CLIP images, extras) per length: what _decode_batch takes."""
    out = []
    for s, L in enumerate(lengths):
        b = OM.make_batch(cfg, 1, seed=s, L=L)
        out.append((np.asarray(b["input_ids"]).astype(np.int64), b["images_clip"].to(torch.bfloat16).to(dev), G.NO_EXTRAS))
    return out


def _padded(prompts):
    """The prompts as generate()'s arguments: right-padded ids, attention mask, stacked images."""
    width = max(p[0].shape[1] for p in prompts)
    ids, att = np.zeros((len(prompts), width), dtype=np.int64), np.zeros((len(prompts), width), dtype=np.int64)
    for r, p in enumerate(prompts):
        ids[r, :p[0].shape[1]], att[r, :p[0].shape[1]] = p[0][0], 1
    return ids, torch.cat([p[1] for p in prompts]), att


class _ScriptedRows:
    """Teacher forcing of a batch: token `step` of row b is script[b, step]."""
    needs_step = True

    def __init__(self, script, dev):
        self.script = torch.as_tensor(np.asarray(script), dtype=torch.int64).to(dev)

    def __call__(self, logits, step):
        if torch.is_tensor(step):
            return self.script.index_select(1, step).reshape(-1)
        return self.script[:, int(step)].clone()


def _run(m, prompts, graph, batch_prefill=True, pick=G._argmax_pick, n_new=N_NEW):
    """One batch decode -> ([ids per row], [[hidden of the prompt [S, d], hidden [d] of every fed token] per row] on the host)."""
    m.decode_with_graph = graph
    with m._decoding("test"):
        for generated, _, hiddens in m._decode_batch(prompts, n_new, (), pick=pick, batch_prefill=batch_prefill):
            pass
    torch.cuda.synchronize()
    assert m.last_decode_path == ("graph" if graph else "loop")
    return [list(g) for g in generated], [[hs[0][0].float().cpu()] + [h.reshape(-1).float().cpu() for h in hs[1:]] for hs in hiddens]


def _single(m, prompt, graph=True, n_new=N_NEW):
    m.decode_with_graph = graph
    with m._decoding("test"):
        for generated, _, hiddens in m._decode(prompt[0], prompt[1], n_new, ()):
            pass
    return list(generated), [h.reshape(-1).float().cpu() for h in hiddens[1:]]


def _equal_runs(a, b, rows_a, rows_b):
    """Tokens, the prompt's hidden states and every fed token's: equal."""
    for ra, rb in zip(rows_a, rows_b):
        assert a[0][ra] == b[0][rb], (ra, rb)
        assert len(a[1][ra]) == len(b[1][rb]) == N_NEW and all(torch.equal(x, y) for x, y in zip(a[1][ra], b[1][rb])), (ra, rb)


def _segmented_pass(m, prompts, **kw):
    """The prompts through LlamaStack.forward(seg_lens=) as _prefill_batch(batched=True) stacks them -> (forward's triple, lengths, cache, the stacked embeddings)."""
    llm = m.model.llm
    planned = [m._plan_embeds(*p) for p in prompts]
    lengths = [S for _, S in planned]
    embeds = torch.zeros((len(prompts), max(lengths), m.config.hidden_size), dtype=torch.bfloat16, device=planned[0][0].device)
    for b, (row, S) in enumerate(planned):
        embeds[b, :S].copy_(row[0])
    cache = llm.new_kv_cache(len(prompts), max(lengths) + 1)
    return llm.forward(embeds, kv_cache=cache, seg_lens=lengths, **kw), lengths, cache, embeds


def _count_calls(monkeypatch, name):
    n = [0]
    orig = getattr(ops, name)

    def counted(*a, **kw):
        n[0] += 1
        return orig(*a, **kw)
    monkeypatch.setattr(ops, name, counted)
    return n


@pytest.mark.parametrize("kind", KINDS)
def test_a_group_of_one_is_the_per_row_prefill(dev, kind):
    cfg, m = _tiny(dev, kind)
    p = _prompts(cfg, dev)
    _equal_runs(_run(m, p[1:2], True, batch_prefill=True), _run(m, p[1:2], True, batch_prefill=False), (0,), (0,))


@pytest.mark.parametrize("kind,factor", [(k, None) for k in KINDS] + [(k, 0.5) for k in MOE])
def test_batch_mates_do_not_matter(dev, kind, factor):
    """Rows [p0, p1, p2] against [p2, p0, p1] (same B, same Smax): every row bit-equal, also where the prompts' own capacities drop tokens —
    routing the padded batch as one pass hands a prompt's expert slots to whoever stands in front of it."""
    cfg, m = _tiny(dev, kind, **({} if factor is None else {"eval_capacity_factor": factor}))
    p = _prompts(cfg, dev)
    if factor is not None:                   # (or the case shows nothing: every prompt loses an entry in some layer)
        (_, _, routing), lengths, _, _ = _segmented_pass(m, p, collect_routing=True)
        top_k, T = cfg.top_k_experts, len(p) * max(lengths)
        for b, S in enumerate(lengths):
            assert any(bool((slot[c * T + b * max(lengths):c * T + b * max(lengths) + S] < 0).any())
                       for _, slot, _ in routing for c in range(top_k)), b
    a = _run(m, [p[0], p[1], p[2]], True)
    b = _run(m, [p[2], p[0], p[1]], True)
    assert all(len(t) == N_NEW for t in a[0])
    _equal_runs(a, b, (0, 1, 2), (1, 2, 0))
    assert a[0][0] != a[0][1]                    # (different prompts, different answers)


@pytest.mark.parametrize("kind,factor", [(k, f) for k in MOE for f in (2.0, 0.5)])
def test_each_layer_routes_each_prompt_alone(dev, kind, factor):
    """Layer-local, so near-tied gates cannot compound: every MoE layer's recorded routing against rmsnorm -> moe_gate -> the unsegmented
    routing op on that layer's own gate input, prompt by prompt at capacity(S_b): expert ids, the dropped set and the slot ranks behind the
    earlier prompts' kept rows, equal."""
    cfg, m = _tiny(dev, kind, eval_capacity_factor=factor)
    llm = m.model.llm
    p = _prompts(cfg, dev)
    (hidden, aux, routing), lengths, cache, embeds = _segmented_pass(m, p, collect_routing=True)
    top_k, E, Smax = cfg.top_k_experts, cfg.num_experts, max(lengths)
    T = len(p) * Smax
    moe_layers = sorted(llm.moe_layers)
    assert len(routing) == len(aux) == len(llm.last_gate_inputs) == len(moe_layers) > 0 and cache["len"] == Smax
    for (expert, slot, counts), l_aux, x_in, i in zip(routing, aux, llm.last_gate_inputs, moe_layers):
        lw = llm.layers[i]
        assert expert.shape == slot.shape == (top_k * T,) and l_aux.shape == (len(p),)
        base = torch.zeros(E, dtype=torch.int64, device=dev)
        total = torch.zeros(E, dtype=torch.int64, device=dev)
        for b, S in enumerate(lengths):
            h = ops.rmsnorm(x_in[b * Smax:b * Smax + S].contiguous(), lw["ln2"], cfg.rms_norm_eps)
            logits, gates = ops.moe_gate(h, lw["wg"])
            if top_k == 1:
                r_expert, r_slot, _, r_kept, r_counts, r_aux = ops.moe_route_top1(gates, llm.capacity(S))
            else:
                r_expert, r_slot, _, r_kept, r_counts, r_aux = ops.moe_route_top2(gates, logits, llm.capacity(S))
            for c in range(top_k):
                mine, ref = slice(c * T + b * Smax, c * T + b * Smax + S), slice(c * S, (c + 1) * S)
                dropped = r_slot[ref] < 0
                assert torch.equal(expert[mine], r_expert[ref]), (i, b, c)
                assert torch.equal(slot[mine] < 0, dropped), (i, b, c)
                assert torch.equal(slot[mine].long(), torch.where(dropped, r_slot[ref].long(), r_slot[ref].long() + base[r_expert[ref].long()])), (i, b, c)
                pad = slice(c * T + b * Smax + S, c * T + (b + 1) * Smax)
                assert bool((slot[pad] == -1).all()) and bool((expert[pad] == 0).all())
            assert torch.equal(l_aux[b:b + 1], r_aux), (i, b)
            base += r_kept.long()
            total += r_counts
        assert torch.equal(counts, total)
        if factor == 0.5:
            assert bool((slot.view(top_k, len(p), Smax)[:, :, :min(lengths)] < 0).any())
    # a pad row is a residual-only row of every MLP: finite all the way, and what it holds never reaches a real row (test_batch_mates_do_not_matter)
    assert bool(torch.isfinite(hidden.float()).all())


@pytest.mark.parametrize("kind", KINDS)
def test_graph_equals_loop_after_a_batched_prefill(dev, kind):
    cfg, m = _tiny(dev, kind)
    p = _prompts(cfg, dev)
    _equal_runs(_run(m, p, True), _run(m, p, False), (0, 1, 2), (0, 1, 2))


def test_a_dense_row_is_the_single_prompt_model(dev):
    """Teacher-forced with the tokens each prompt gets alone: every row's per-step hidden state within 2^-5 of the largest entry of the
    single-prompt run's, on every step — what the dense case of test_a_row_is_the_single_prompt_model holds the per-row prefill to."""
    cfg, m = _tiny(dev, "dense")
    p = _prompts(cfg, dev)
    alone = [_single(m, q) for q in p]
    pick = _ScriptedRows([t for t, _ in alone], dev)
    for graph in (True, False):
        toks, hid = _run(m, p, graph, pick=pick)
        assert toks == [t for t, _ in alone]
        for r in range(len(p)):
            rel = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(hid[r][1:], alone[r][1])]
            print("graph" if graph else "loop", f"row {r}: worst {max(rel):.5f} of the max entry")
            assert len(rel) == N_NEW - 1 and all(x <= BOUND for x in rel), rel


@pytest.mark.parametrize("kind", KINDS)
def test_passes_and_launches(dev, kind, monkeypatch):
    cfg, m = _tiny(dev, kind)
    llm = m.model.llm
    p = _prompts(cfg, dev)
    seg = {k: _count_calls(monkeypatch, n) for k, n in SEGMENTED.items()}
    plain = [_count_calls(monkeypatch, n) for n in ("moe_route_top1", "moe_route_top2")]
    moe_layers = len(llm.moe_layers) if kind != "dense" else 0
    pass0 = llm.gate_pass
    with m._decoding("test"):
        hiddens, cache, lengths = m._prefill_batch(p, 4, batched=True)
    assert llm.gate_pass - pass0 == 1 and cache["len"] == max(lengths)
    assert [tuple(h.shape) for h in hiddens] == [(1, S, cfg.hidden_size) for S in lengths]
    assert sum(n[0] for n in seg.values()) == moe_layers and (kind == "dense" or seg[kind][0] == moe_layers > 0)
    assert all(n[0] == 0 for n in plain)
    for graph in (True, False):
        pass0 = llm.gate_pass
        _run(m, p, graph)
        assert llm.gate_pass - pass0 == 1 + N_NEW - 1
    seen = [n[0] for n in seg.values()]
    pass0 = llm.gate_pass
    _run(m, p, True, batch_prefill=False)
    assert [n[0] for n in seg.values()] == seen and llm.gate_pass - pass0 == len(p) + N_NEW - 1


def _expected_layout(prompts, script, n_new):
    rows = []
    for p, s in zip(prompts, script):
        s = list(s[:n_new])
        ans = s[:s.index(EOS) + 1] if EOS in s else s
        rows.append(list(p[0][0]) + ans)
    width = max(len(r) for r in rows)
    return torch.tensor([r + [EOS] * (width - len(r)) for r in rows])


@pytest.mark.parametrize("kind", ("dense", "top1"))
def test_rows_stop_on_their_own(dev, kind):
    cfg, m = _tiny(dev, kind)
    p = _prompts(cfg, dev)
    ids, clip, att = _padded(p)
    llm = m.model.llm
    g = torch.Generator().manual_seed(9)
    script = torch.randint(3, 100, (3, 40), generator=g).numpy()
    first = script.copy()
    first[0, 1] = EOS                            # step 2 of row 0
    first[2, 15] = EOS                           # step 16, the last, of row 2; never in row 1
    second = script.copy()
    second[0, 16] = second[2, 16] = EOS          # step 17 of 40: a look boundary
    second[1, 4] = EOS
    for sc, n_new, steps in ((first, 16, 16), (second, 40, 17)):
        passes = []
        for graph in (True, False):
            m.decode_with_graph = graph
            pass0 = llm.gate_pass
            out = m._generate_groups(ids, clip, att, n_new, EOS, 8, {}, _ScriptedRows(sc, dev), batch_prefill=True)
            assert m.last_decode_path == ("graph" if graph else "loop")
            assert torch.equal(out, _expected_layout(p, sc, n_new)), (graph, out)
            passes.append(llm.gate_pass - pass0)
        assert passes[0] == passes[1] == 1 + steps - 1, passes       # one prefill pass for the group; gate_pass ends where the loop leaves it


def test_refusals(dev):
    cfg, m = _tiny(dev, "top1")
    llm = m.model.llm
    p = _prompts(cfg, dev)
    (_, _, _), lengths, cache, embeds = _segmented_pass(m, p)
    Smax = max(lengths)
    pass0 = llm.gate_pass

    def fresh():
        return llm.new_kv_cache(len(p), Smax + 1)
    with pytest.raises(ValueError, match="seg_lens"):
        llm.forward(embeds, torch.ones((len(p), Smax), dtype=torch.uint8, device=dev), kv_cache=fresh(), seg_lens=lengths)
    with pytest.raises(ValueError, match="seg_lens"):
        llm.forward(embeds, kv_cache=cache, seg_lens=lengths)                   # not empty: the pass above filled it
    with pytest.raises(ValueError, match="seg_lens"):
        llm.forward(embeds, seg_lens=lengths)                                   # no cache at all
    for bad in ([0] + lengths[1:], lengths[:-1] + [Smax + 1], lengths[:-1]):
        with pytest.raises(ValueError, match="seg_lens"):
            llm.forward(embeds, kv_cache=fresh(), seg_lens=bad)
    llm.rts_uniform_provider = lambda i, T, E: torch.full((T * E,), 0.5, dtype=torch.float32, device=dev)
    with pytest.raises(NotImplementedError, match="draw provider"):
        llm.forward(embeds, kv_cache=fresh(), seg_lens=lengths)
    llm.rts_uniform_provider = None
    llm.cfg.moe_gate_sampling = True
    with pytest.raises(NotImplementedError, match="moe_gate_sampling"):
        llm.forward(embeds, kv_cache=fresh(), seg_lens=lengths)
    ids, clip, att = _padded(p)
    with pytest.raises(NotImplementedError, match="moe_gate_sampling"):
        m.generate_batch(ids, images=clip, attention_mask=att, max_new_tokens=4, eos_token_id=-1, batch_prefill=True)
    llm.cfg.moe_gate_sampling = False
    assert llm.gate_pass == pass0
    cfg, m = _tiny(dev, "top1", use_residual=True)
    llm = m.model.llm
    pass0 = llm.gate_pass
    with pytest.raises(NotImplementedError, match="use_residual"):
        llm.forward(embeds, kv_cache=llm.new_kv_cache(len(p), Smax + 1), seg_lens=lengths)
    assert llm.gate_pass == pass0


def test_sampled_and_streamed_groups_take_the_switch(dev, monkeypatch):
    """generate_sample_batch(batch_prefill=True) and generate_stream_batch under model.stream_batch_prefill: one segmented routing call per
    MoE layer and group, none with the switch off; greedy streamed rows are generate_batch(batch_prefill=True)'s tokens."""
    cfg, m = _tiny(dev, "top1")
    p = _prompts(cfg, dev)
    ids, clip, att = _padded(p)
    moe_layers = len(m.model.llm.moe_layers)
    segmented = _count_calls(monkeypatch, SEGMENTED["top1"])
    for on in (False, True):
        seen = segmented[0]
        out = m.generate_sample_batch(ids, images=clip, attention_mask=att, max_new_tokens=4, eos_token_id=-1, sample_seed=5, batch_prefill=on)
        assert out.shape == (3, max(q[0].shape[1] for q in p) + 4) and segmented[0] - seen == (moe_layers if on else 0)
    greedy = m.generate_batch(ids, images=clip, attention_mask=att, max_new_tokens=4, eos_token_id=-1, batch_prefill=True)
    requests = [G.StreamRequest(input_ids=q[0], images_clip=q[1], temperature=0.0, max_new_tokens=4) for q in p]
    assert m.stream_batch_prefill is False
    for on in (False, True):
        m.stream_batch_prefill = on
        seen, last = segmented[0], {}
        for row, new, stopped, _ in m.generate_stream_batch(requests, eos_token_id=-1):
            last[row] = new
        assert segmented[0] - seen == (moe_layers if on else 0) and sorted(last) == [0, 1, 2]
    for r, q in enumerate(p):
        L = q[0].shape[1]
        assert last[r] == greedy[r, L:L + 4].tolist(), r


def test_infer_driver_prefills_in_batches(dev, tmp_path, monkeypatch):
    from medplib_amd import infer
    from medplib_amd.train import SyntheticDataset
    cfg, m = _tiny(dev, "top1")
    val = SyntheticDataset(cfg, 1, 3, 49, True)
    segmented = _count_calls(monkeypatch, SEGMENTED["top1"])
    calls = []
    orig = m._prefill_batch

    def prefill(prompts, max_new_tokens, batched=False):
        calls.append((len(prompts), bool(batched)))
        return orig(prompts, max_new_tokens, batched=batched)
    monkeypatch.setattr(m, "_prefill_batch", prefill)
    records = {}
    for on in (True, False):
        path = tmp_path / f"answers_{int(on)}.jsonl"
        seen = segmented[0]
        outs = infer.run_vqa(val, m, dev, max_new_tokens=5, answers_file=str(path), decode_batch=3, prefill_batch=on)
        assert len(outs) == 3 and calls[-1] == (3, on)
        assert segmented[0] - seen == (len(m.model.llm.moe_layers) if on else 0)
        records[on] = [json.loads(line) for line in open(path)]
    assert [r["question_id"] for r in records[True]] == [r["question_id"] for r in records[False]] == [0, 1, 2]
    assert all(set(a) == set(b) and 1 <= len(a["output_ids"]) <= 5 for a, b in zip(records[True], records[False]))
    with pytest.raises(ValueError, match="--prefill_batch"):
        infer.run_vqa(val, m, dev, max_new_tokens=5, decode_batch=1, prefill_batch=True)
