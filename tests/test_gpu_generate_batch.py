"""generate_batch(): ragged prompts as the rows of one decode step, on the tiny config (dense, E = 2 top-1, E = 2 top-2).  A row of a batch is
the single-prompt model in another summation order, so rows are compared with generate() through teacher-forced hidden states and the
project's bound for that; no test compares TOKENS of the batch and the single-prompt path on random tiny weights (the docstring of
tests/test_gpu_quant_decode.py says why).  What must be exact — the order of the rows, graph against loop, the output layout — is."""
import json
import statistics

import numpy as np
import pytest
import torch

from medplib_amd import ops
from medplib_amd.model import generation as G
from medplib_amd.model.config import MedPLIBConfig
from oracle import model as OM

pytestmark = pytest.mark.gpu

KINDS = ("dense", "top1", "top2")
N_NEW = 16
BOUND = 2.0 ** -5            # "same function, another summation order" (BOUND of tests/test_gpu_quant_decode.py)
LENGTHS = (24, 31, 17)
EOS = 2


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
    """Teacher forcing of a batch: token `step` of row b is script[b, step] (tests/test_gpu_quant_decode.py's _ScriptedPick over [B, n])."""
    needs_step = True

    def __init__(self, script, dev):
        self.script = torch.as_tensor(np.asarray(script), dtype=torch.int64).to(dev)

    def __call__(self, logits, step):
        if torch.is_tensor(step):
            return self.script.index_select(1, step).reshape(-1)
        return self.script[:, int(step)].clone()


def _run(m, prompts, graph, pick=G._argmax_pick, n_new=N_NEW, stop=()):
    """One batch decode -> ([ids per row], [[hidden [d] of every fed token] per row] on the host); asserts the path taken."""
    m.decode_with_graph = graph
    with m._decoding("test"):
        for generated, _, hiddens in m._decode_batch(prompts, n_new, stop, pick=pick):
            pass
    torch.cuda.synchronize()
    assert m.last_decode_path == ("graph" if graph else "loop")
    return [list(g) for g in generated], [[h.reshape(-1).float().cpu() for h in hs[1:]] for hs in hiddens]


def _single(m, prompt, graph=True, n_new=N_NEW):
    m.decode_with_graph = graph
    with m._decoding("test"):
        for generated, _, hiddens in m._decode(prompt[0], prompt[1], n_new, ()):
            pass
    return list(generated), [h.reshape(-1).float().cpu() for h in hiddens[1:]]


def _equal_runs(a, b, rows_a, rows_b):
    for ra, rb in zip(rows_a, rows_b):
        assert a[0][ra] == b[0][rb], (ra, rb)
        assert len(a[1][ra]) == len(b[1][rb]) == N_NEW - 1 and all(torch.equal(x, y) for x, y in zip(a[1][ra], b[1][rb])), (ra, rb)


@pytest.mark.parametrize("kind,mode", [(k, "bf16") for k in KINDS] + [(k, q) for k in ("dense", "top1") for q in ("w8", "w4")])
def test_order_of_the_rows_does_not_matter(dev, kind, mode):
    cfg, m = _tiny(dev, kind)
    if mode == "w8":
        m.enable_decode_8bit(True)
    elif mode == "w4":
        m.enable_decode_4bit(True)
    p = _prompts(cfg, dev)
    a = _run(m, [p[0], p[1], p[2]], True)
    b = _run(m, [p[2], p[0], p[1]], True)
    assert all(len(t) == N_NEW for t in a[0])
    _equal_runs(a, b, (0, 1, 2), (1, 2, 0))
    assert a[0][0] != a[0][1]                    # (different prompts, different answers)


@pytest.mark.parametrize("kind", KINDS)
def test_graph_equals_loop(dev, kind):
    cfg, m = _tiny(dev, kind)
    p = _prompts(cfg, dev)
    llm = m.model.llm
    pass0 = llm.gate_pass
    a = _run(m, p, True)
    passes_graph = llm.gate_pass - pass0
    b = _run(m, p, False)
    assert llm.gate_pass - pass0 == 2 * passes_graph == 2 * (len(p) + N_NEW - 1)       # a prefill per row, then one pass per fed token
    _equal_runs(a, b, (0, 1, 2), (0, 1, 2))
    one = _run(m, p[1:2], True)                  # a group of one takes the same path
    assert len(one[0]) == 1 and len(one[0][0]) == N_NEW


@pytest.mark.parametrize("kind", KINDS)
def test_a_row_is_the_single_prompt_model(dev, kind):
    """Teacher-forced with the tokens each prompt gets alone: every row's per-step hidden state within 2^-5 of the largest entry of the
    single-prompt run's; MoE kinds may miss it on at most two steps per prompt (a near-tied gate sends a step to the other expert)."""
    cfg, m = _tiny(dev, kind)
    p = _prompts(cfg, dev)
    alone = [_single(m, q) for q in p]
    pick = _ScriptedRows([t for t, _ in alone], dev)
    for graph in (True, False):
        toks, hid = _run(m, p, graph, pick=pick)
        assert toks == [t for t, _ in alone]
        for r in range(len(p)):
            rel = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(hid[r], alone[r][1])]
            print(kind, "graph" if graph else "loop", f"row {r}: worst {max(rel):.5f} median {statistics.median(rel):.5f} of the max entry")
            assert len(rel) == N_NEW - 1 and sum(x > BOUND for x in rel) <= (0 if kind == "dense" else 2), rel


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
            out = m._generate_groups(ids, clip, att, n_new, EOS, 8, {}, _ScriptedRows(sc, dev))      # (generate_batch behind its argument checks)
            assert m.last_decode_path == ("graph" if graph else "loop")
            assert torch.equal(out, _expected_layout(p, sc, n_new)), (graph, out)
            passes.append(llm.gate_pass - pass0)
        assert passes[0] == passes[1] == len(p) + steps - 1, passes       # gate_pass ends where the loop leaves it


def test_groups_of_batch_rows(dev):
    cfg, m = _tiny(dev, "top1")
    p = _prompts(cfg, dev, (24, 31, 17, 28, 20))
    ids, clip, att = _padded(p)
    out = m.generate_batch(ids, images=clip, attention_mask=att, max_new_tokens=8, eos_token_id=-1, batch_rows=2)
    assert out.shape == (5, 31 + 8)
    for lo, hi in ((0, 2), (2, 4), (4, 5)):
        gi, gc, ga = _padded(p[lo:hi])
        by_hand = m.generate_batch(gi, images=gc, attention_mask=ga, max_new_tokens=8, eos_token_id=-1, batch_rows=2)
        for r in range(lo, hi):
            n = p[r][0].shape[1] + 8
            assert torch.equal(out[r, :n], by_hand[r - lo, :n]) and bool((out[r, n:] == -1).all())
    for bad in (0, 9):
        with pytest.raises(ValueError):
            m.generate_batch(ids, images=clip, attention_mask=att, max_new_tokens=8, batch_rows=bad)


def _count_calls(monkeypatch, name, when=lambda a, kw: True):
    n = [0]
    orig = getattr(ops, name)

    def counted(*a, **kw):
        n[0] += bool(when(a, kw))
        return orig(*a, **kw)
    monkeypatch.setattr(ops, name, counted)
    return n


def test_launches_of_a_top1_batch(dev, monkeypatch):
    cfg, m = _tiny(dev, "top1")
    p = _prompts(cfg, dev, (24, 31, 17, 28))
    ids, clip, att = _padded(p)
    grouped = _count_calls(monkeypatch, "gemv_grouped")
    indexed = _count_calls(monkeypatch, "gemv", lambda a, kw: kw.get("w_index") is not None)
    rope_rows = _count_calls(monkeypatch, "decode_rope_append_rows")
    attn_rows = _count_calls(monkeypatch, "attention_decode_rows")
    fused = [_count_calls(monkeypatch, n) for n in ("gemv_rmsnorm_rope_append", "gemv_rmsnorm", "decode_rope_append")]
    moe_layers = len(m.model.llm.moe_layers)
    assert moe_layers > 0
    for graph in (True, False):
        m.decode_with_graph = graph
        seen = (grouped[0], rope_rows[0], attn_rows[0])
        m.generate_batch(ids, images=clip, attention_mask=att, max_new_tokens=4, eos_token_id=-1)
        steps = 1 if graph else 3                # (captured: the launches are recorded once)
        assert grouped[0] - seen[0] == 2 * moe_layers * steps
        assert rope_rows[0] - seen[1] == attn_rows[0] - seen[2] == len(m.model.llm.layers) * steps
        assert indexed[0] == 0 and all(f[0] == 0 for f in fused)
    m.model.llm.group_expert_gemvs = False       # the A/B switch: the indexed form
    seen = grouped[0]
    m.generate_batch(ids, images=clip, attention_mask=att, max_new_tokens=4, eos_token_id=-1)
    assert grouped[0] == seen and indexed[0] > 0


def test_refusals_leave_the_model_decoding_as_before(dev):
    def refused(m, cfg, match, **kw):
        p = _prompts(cfg, dev)
        ids, clip, att = _padded(p)
        before = m.generate(ids, images=clip, attention_mask=att, max_new_tokens=4, eos_token_id=-1)
        pass0, training = m.model.llm.gate_pass, m.training
        with pytest.raises(NotImplementedError, match=match):
            m.generate_batch(ids, images=clip, attention_mask=att, max_new_tokens=4, eos_token_id=-1, **kw)
        assert m.model.llm.gate_pass == pass0 and m.training == training
        assert torch.equal(m.generate(ids, images=clip, attention_mask=att, max_new_tokens=4, eos_token_id=-1), before)

    cfg, m = _tiny(dev, "top1")
    llm = m.model.llm
    refused(m, cfg, "generate_sample", do_sample=True)
    refused(m, cfg, "generate_beam", num_beams=2)
    # an injected draw provider (the same draws at every pass, so generate() before and after can be compared)
    llm.rts_uniform_provider = lambda i, T, E: torch.full((T * E,), 0.5, dtype=torch.float32, device=dev)
    refused(m, cfg, "draw provider")
    llm.rts_uniform_provider = None
    llm.cfg.moe_gate_sampling = True             # (its draws are keyed on the pass number: only the refusal itself is checked)
    pass0 = llm.gate_pass
    ids, clip, att = _padded(_prompts(cfg, dev))
    with pytest.raises(NotImplementedError, match="moe_gate_sampling"):
        m.generate_batch(ids, images=clip, attention_mask=att, max_new_tokens=4, eos_token_id=-1)
    with pytest.raises(NotImplementedError, match="moe_gate_sampling"):      # the stack refuses too, before it counts a pass
        llm.decode_step(None, None, None, rows=(None, None))
    assert llm.gate_pass == pass0
    cfg, m = _tiny(dev, "top1", use_residual=True)
    refused(m, cfg, "use_residual")


def test_infer_driver_decodes_in_batches(dev, tmp_path):
    from medplib_amd import infer
    records = {}
    for n in (2, 1):
        path = tmp_path / f"answers_{n}.jsonl"
        out = infer.main(["--model_size", "tiny", "--n_samples", "3", "--max_new_tokens", "5", "--eval_vqa", "--decode_batch", str(n),
                          "--answers_file", str(path)])
        assert len(out["vqa_output_ids"]) == 3
        records[n] = [json.loads(line) for line in open(path)]
    assert [r["question_id"] for r in records[2]] == [r["question_id"] for r in records[1]] == [0, 1, 2]
    assert all(set(a) == set(b) and 1 <= len(a["output_ids"]) <= 5 for a, b in zip(records[2], records[1]))


def test_infer_driver_cuts_ragged_answers_as_generate_does(dev):
    """Prompts of different lengths in one group, an eos that one row meets and the others do not: every sample's ids are its prompt and its
    answer alone — cut after its own eos, or max_new_tokens ids without one — with nothing of the group's eos padding, as generate() returns
    them for the sample alone (same length, same layout)."""
    from medplib_amd import infer
    cfg, m = _tiny(dev, "top1")
    n_new, lengths = 6, (31, 17, 24)             # the widest row first: the others are padded on the right
    samples = []
    for s_, L in enumerate(lengths):
        b = OM.make_batch(cfg, 1, seed=s_, L=L)
        samples.append({"input_ids": b["input_ids"], "attention_mask": b["attention_mask"], "images_clip": b["images_clip"].to(torch.bfloat16).to(dev)})
    free = infer._generate_together(m, samples, list(lengths), n_new, eos=-1)          # no row stops: the batch path's own tokens
    assert [r.shape for r in free] == [(1, L + n_new) for L in lengths]
    answers = [r[0, L:].tolist() for r, L in zip(free, lengths)]
    # an eos that row 0 produces as its fourth token at the latest and the shorter rows never do
    eos = next(t for t in answers[0][1:4] if t not in answers[1] and t not in answers[2])
    stop0 = answers[0].index(eos) + 1
    got = infer._generate_together(m, samples, list(lengths), n_new, eos=eos)
    want = [answers[0][:stop0], answers[1], answers[2]]
    for r, (b, L) in enumerate(zip(samples, lengths)):
        assert got[r].shape == (1, L + len(want[r])), (r, got[r].shape)
        assert got[r][0, :L].tolist() == b["input_ids"][0].tolist() and got[r][0, L:].tolist() == want[r]
        alone = m.generate(b["input_ids"], images=b["images_clip"], attention_mask=b["attention_mask"], max_new_tokens=n_new, eos_token_id=eos)
        assert alone.shape == got[r].shape and (int(alone[0, -1]) == eos) == (int(got[r][0, -1]) == eos) == (r == 0)
    with pytest.raises(NotImplementedError, match="image_token_lengths"):
        infer._generate_together(m, [dict(samples[0], image_token_lengths=[[4]])], [31], n_new)
