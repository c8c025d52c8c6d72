"""generate_batch() under the quantised decode modes on a top-1 MoE model (tiny config, E = 2): the rows of a batch that name the same expert
share one pass over its int8 / NF4 copies (ops.gemv_grouped_w8 / ops.gemv_grouped_w4).  The grouped op has the indexed op's bits, so switching
it off (group_expert_gemvs = False) changes no token and no logit; which op is launched, and how often, is counted."""
import numpy as np
import pytest
import torch

from medplib_amd import ops
from medplib_amd.model import generation as G
from medplib_amd.model.config import MedPLIBConfig
from medplib_amd.model.llama import DECODE_MODES
from oracle import model as OM

pytestmark = pytest.mark.gpu

BITS = (8, 4)
LENGTHS = (24, 31, 17, 28)
N_NEW = 8
GROUPED_OPS = ("gemv_grouped", "gemv_grouped_w8", "gemv_grouped_w4")


def _tiny(dev):
    from medplib_amd.model.medplib import MedPLIBForCausalLM
    cfg = MedPLIBConfig.tiny(moe_enable=True, sam_depth=2, num_experts=2, top_k_experts=1)
    m = MedPLIBForCausalLM(cfg, device=dev)
    m.load_hf_state_dict(OM.init_hf_weights(cfg, seed=3))
    return cfg, m.eval()


def _enable(m, bits, on=True):
    getattr(m, f"enable_decode_{bits}bit")(on)


def _prompts(cfg, dev):
    out = []
    for s, L in enumerate(LENGTHS):
        b = OM.make_batch(cfg, 1, seed=s, L=L)
        out.append((np.asarray(b["input_ids"]).astype(np.int64), b["images_clip"].to(torch.bfloat16).to(dev), G.NO_EXTRAS))
    return out


def _padded(prompts):
    width = max(p[0].shape[1] for p in prompts)
    ids, att = np.zeros((len(prompts), width), dtype=np.int64), np.zeros((len(prompts), width), dtype=np.int64)
    for r, p in enumerate(prompts):
        ids[r, :p[0].shape[1]], att[r, :p[0].shape[1]] = p[0][0], 1
    return ids, torch.cat([p[1] for p in prompts]), att


def _run(m, prompts, graph):
    """One batch decode -> ([ids per row], [(fp32 logits [B, V], the B tokens) per step])."""
    m.decode_with_graph = graph
    debug = []
    with m._decoding("test"):
        for generated, _, _ in m._decode_batch(prompts, N_NEW, (), debug=debug):
            pass
    torch.cuda.synchronize()
    assert m.last_decode_path == ("graph" if graph else "loop")
    return [list(g) for g in generated], debug


@pytest.mark.parametrize("bits", BITS)
def test_grouped_and_indexed_batches_agree_bit_for_bit(dev, bits):
    cfg, m = _tiny(dev)
    _enable(m, bits)
    p = _prompts(cfg, dev)
    llm = m.model.llm
    for graph in (True, False):
        runs = []
        for grouped in (True, False):
            llm.group_expert_gemvs = grouped
            runs.append(_run(m, p, graph))
        (tok_a, dbg_a), (tok_b, dbg_b) = runs
        assert tok_a == tok_b and all(len(t) == N_NEW for t in tok_a)
        assert len(dbg_a) == len(dbg_b) == N_NEW
        for step, ((la, ta), (lb, tb)) in enumerate(zip(dbg_a, dbg_b)):
            assert la.shape == (len(p), cfg.vocab_size) and ta == tb
            assert torch.equal(la.view(torch.int32), lb.view(torch.int32)), f"{bits}-bit, graph={graph}: logits of step {step} differ"
        assert tok_a[0] != tok_a[1]                  # (different prompts, different answers)


def _count_calls(monkeypatch, name, when=lambda a, kw: True):
    n = [0]
    orig = getattr(ops, name)

    def counted(*a, **kw):
        n[0] += bool(when(a, kw))
        return orig(*a, **kw)
    monkeypatch.setattr(ops, name, counted)
    return n


@pytest.mark.parametrize("bits", BITS)
def test_launches_of_a_quantised_top1_batch(dev, monkeypatch, bits):
    cfg, m = _tiny(dev)
    mode = DECODE_MODES[bits]
    p = _prompts(cfg, dev)
    ids, clip, att = _padded(p)
    grouped = {n: _count_calls(monkeypatch, n) for n in GROUPED_OPS}
    indexed = _count_calls(monkeypatch, mode.gemv, lambda a, kw: kw.get("w_index") is not None)
    indexed_bf16 = _count_calls(monkeypatch, "gemv", lambda a, kw: kw.get("w_index") is not None)
    others = [grouped[n] for n in GROUPED_OPS if n != mode.gemv_grouped]
    mine = grouped[mode.gemv_grouped]
    llm = m.model.llm
    moe_layers = len(llm.moe_layers)
    assert moe_layers > 0
    _enable(m, bits)
    for graph in (True, False):
        m.decode_with_graph = graph
        seen = mine[0]
        m.generate_batch(ids, images=clip, attention_mask=att, max_new_tokens=4, eos_token_id=-1)
        steps = 1 if graph else 3                    # (captured: the launches are recorded once)
        assert mine[0] - seen == 2 * moe_layers * steps
        assert indexed[0] == 0 and indexed_bf16[0] == 0 and all(o[0] == 0 for o in others)
    llm.group_expert_gemvs = False                   # the A/B switch: the indexed form of the mode
    seen = mine[0]
    m.generate_batch(ids, images=clip, attention_mask=att, max_new_tokens=4, eos_token_id=-1)
    assert mine[0] == seen and indexed[0] > 0 and indexed_bf16[0] == 0 and all(o[0] == 0 for o in others)
    llm.group_expert_gemvs = True
    _enable(m, bits, False)                          # the mode off: the bf16 grouped op is back
    seen = (mine[0], indexed[0])
    m.generate_batch(ids, images=clip, attention_mask=att, max_new_tokens=4, eos_token_id=-1)
    assert grouped["gemv_grouped"][0] > 0 and (mine[0], indexed[0]) == seen


@pytest.mark.parametrize("bits", BITS)
def test_generate_on_one_prompt_calls_no_grouped_op(dev, monkeypatch, bits):
    cfg, m = _tiny(dev)
    p = _prompts(cfg, dev)
    ids, clip, att = _padded(p[:1])
    grouped = [_count_calls(monkeypatch, n) for n in GROUPED_OPS]
    indexed = _count_calls(monkeypatch, DECODE_MODES[bits].gemv, lambda a, kw: kw.get("w_index") is not None)
    _enable(m, bits)
    for graph in (True, False):
        m.decode_with_graph = graph
        m.generate(ids, images=clip, attention_mask=att, max_new_tokens=4, eos_token_id=-1)
    assert indexed[0] > 0 and all(g[0] == 0 for g in grouped)
