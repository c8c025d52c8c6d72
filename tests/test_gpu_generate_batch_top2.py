"""generate_batch() on top-2 models: the (row, choice) entries of a ragged step share one weight pass per expert (ops.gemv_grouped_top2_gate_up /
ops.gemv_grouped_top2_down).  The grouped kernels are bit-identical with the per-entry pair, so group_expert_gemvs True against False is
compared EXACTLY — tokens and every per-step hidden state, captured and looped — and the launches are counted by patching `ops`.  Tiny config,
E = 2 (every token names both experts) and E = 3."""
import pytest
import torch

from medplib_amd.model.config import MedPLIBConfig
from oracle import model as OM
from test_gpu_generate_batch import N_NEW, _count_calls, _padded, _prompts, _run

pytestmark = pytest.mark.gpu

LENGTHS = (24, 31, 17, 28)
NEW_OPS = ("gemv_grouped_top2_gate_up", "gemv_grouped_top2_down")
PER_ENTRY_OPS = ("gemv_top2_gate_up", "gemv_top2_down")


def _tiny_top2(dev, E):
    from medplib_amd.model.medplib import MedPLIBForCausalLM
    cfg = MedPLIBConfig.tiny(moe_enable=True, sam_depth=2, num_experts=E, top_k_experts=2)
    m = MedPLIBForCausalLM(cfg, device=dev)
    m.load_hf_state_dict(OM.init_hf_weights(cfg, seed=3))
    return cfg, m.eval()


@pytest.mark.parametrize("E", [2, 3])
def test_grouped_and_per_entry_steps_give_the_same_bits(dev, E):
    cfg, m = _tiny_top2(dev, E)
    p = _prompts(cfg, dev, LENGTHS)
    llm = m.model.llm
    assert llm.group_expert_gemvs and len(llm.moe_layers) > 0
    runs = {}
    for grouped in (True, False):
        llm.group_expert_gemvs = grouped
        for graph in (True, False):
            runs[grouped, graph] = _run(m, p, graph)
    base = runs[False, False]                    # the per-entry pair, token by token
    assert all(len(t) == N_NEW for t in base[0]) and base[0][0] != base[0][1]
    for key, (toks, hid) in runs.items():
        assert toks == base[0], key
        for r in range(len(p)):
            assert len(hid[r]) == len(base[1][r]) == N_NEW - 1 and all(torch.equal(a, b) for a, b in zip(hid[r], base[1][r])), (key, r)


@pytest.mark.parametrize("E", [2, 3])
def test_launches_of_a_top2_batch(dev, monkeypatch, E):
    cfg, m = _tiny_top2(dev, E)
    ids, clip, att = _padded(_prompts(cfg, dev, LENGTHS))
    new = [_count_calls(monkeypatch, n) for n in NEW_OPS]
    per_entry = [_count_calls(monkeypatch, n) for n in PER_ENTRY_OPS]
    llm = m.model.llm
    moe_layers = len(llm.moe_layers)
    assert moe_layers > 0

    def ragged_calls(counters):
        """The calls of a generate_batch over four prompts that are not the prefills' (a prefill of 17+ rows takes the GEMM path: none)."""
        seen = [c[0] for c in counters]
        m.generate_batch(ids, images=clip, attention_mask=att, max_new_tokens=4, eos_token_id=-1)
        return [c[0] - s for c, s in zip(counters, seen)]

    for graph in (True, False):
        m.decode_with_graph = graph
        steps = 1 if graph else 3                # (captured: the launches are recorded once)
        seen_old = [c[0] for c in per_entry]
        assert ragged_calls(new) == [moe_layers * steps] * 2
        assert m.last_decode_path == ("graph" if graph else "loop")
        assert [c[0] for c in per_entry] == seen_old, "a ragged step took the per-entry pair"
    # a group of one keeps the per-entry pair (two entries, two experts: the same streams either way, and measured no faster grouped)
    seen_new, seen_old = [c[0] for c in new], [c[0] for c in per_entry]
    m.generate_batch(ids[:1, :LENGTHS[0]], images=clip[:1], attention_mask=att[:1, :LENGTHS[0]], max_new_tokens=4, eos_token_id=-1)
    assert [c[0] for c in new] == seen_new and [c[0] - s for c, s in zip(per_entry, seen_old)] == [moe_layers * 3] * 2
    llm.group_expert_gemvs = False               # the A/B switch: the per-entry pair
    for graph in (True, False):
        m.decode_with_graph = graph
        steps = 1 if graph else 3
        seen_new = [c[0] for c in new]
        assert ragged_calls(per_entry) == [moe_layers * steps] * 2
        assert [c[0] for c in new] == seen_new


def test_non_ragged_paths_keep_the_per_entry_pair(dev, monkeypatch):
    cfg, m = _tiny_top2(dev, 3)
    ids, clip, att = _padded(_prompts(cfg, dev, LENGTHS))
    new = [_count_calls(monkeypatch, n) for n in NEW_OPS]
    per_entry = [_count_calls(monkeypatch, n) for n in PER_ENTRY_OPS]
    assert m.model.llm.group_expert_gemvs
    m.generate(ids, images=clip, attention_mask=att, max_new_tokens=4, eos_token_id=-1)
    assert all(c[0] > 0 for c in per_entry)
    seen = [c[0] for c in per_entry]
    m.generate_beam(ids[:1, :LENGTHS[0]], images=clip[:1], attention_mask=att[:1, :LENGTHS[0]], max_new_tokens=4, eos_token_id=-1, num_beams=4)
    assert all(c[0] > s for c, s in zip(per_entry, seen))
    assert all(c[0] == 0 for c in new)
