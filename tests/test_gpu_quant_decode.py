"""Quantised decode weights through the model (MedPLIBForCausalLM.enable_decode_8bit, the worker's --load-8bit; enable_decode_4bit, NF4) on
the tiny config, dense and E = 2 top-1, every test under both modes (tests/test_gpu_w8_decode.py holds what is 8-bit by name, on these
helpers): with the decoder weights snapped to the quantiser's grid (so code * scale IS the bf16 weight) the quantised model is the SAME
function as the bf16 one (other summation order, unfused norms), so teacher-forced hidden states must agree within the project's bound for that; with random weights it is a different function, namely the bf16 model on the
dequantised weights.  No test here compares TOKENS of a quantised and the bf16 model on random tiny weights: the top-2 logit gaps of such
runs are 0.002-0.05, so a near-tie hatch would swallow every step."""
import collections

import numpy as np
import pytest
import torch

import nf4_ref as R
from medplib_amd import ops
from medplib_amd.model import generation as G
from medplib_amd.model.config import MedPLIBConfig
from oracle import model as OM

pytestmark = pytest.mark.gpu

KINDS = ("dense", "top1")
BITS = (8, 4)
N_NEW = 16
BOUND = 2.0 ** -5            # "same function, another summation order" (test_decode_is_prefix_consistent_and_equals_the_prefill_at_true_dims)
KEYS = ("qkv", "o", "gu", "down")


def _tiny(dev, kind, **kw):
    from medplib_amd.model.medplib import LISAForCausalLM, MedPLIBForCausalLM
    if kind == "dense":
        cfg, cls = MedPLIBConfig.tiny(moe_enable=False, sam_depth=2, **kw), LISAForCausalLM
    else:
        cfg, cls = MedPLIBConfig.tiny(moe_enable=True, sam_depth=2, num_experts=2, top_k_experts=1 if kind == "top1" else 2, **kw), MedPLIBForCausalLM
    W = OM.init_hf_weights(cfg, seed=3)
    m = cls(cfg, device=dev)
    m.load_hf_state_dict(W)
    return cfg, m.eval()


def _inputs(cfg, dev, seed=0):
    b = OM.make_batch(cfg, 1, seed=seed)
    return b, b["images_clip"].to(torch.bfloat16).to(dev), b["images"].to(torch.bfloat16).float().to(dev)


class _ScriptedPick:
    """Teacher forcing: token `step` of the answer is script[step], whatever the logits say.  needs_step: the captured step keeps the token
    number on the device and hands it over as an int32 [1] tensor, the loop hands over an int."""
    needs_step = True

    def __init__(self, script, dev):
        self.script = torch.as_tensor(script, dtype=torch.int64).to(dev)

    def __call__(self, logits, step):
        if torch.is_tensor(step):
            return self.script.index_select(0, step)
        return self.script[int(step):int(step) + 1].clone()


def _run(m, b, clip, graph, pick=G._argmax_pick, n_new=N_NEW):
    """One decode of n_new tokens -> (ids, [hidden [d] of every fed token] on the host); asserts the path taken."""
    m.decode_with_graph = graph
    with m._decoding("test"):
        for generated, _, hiddens in m._decode(np.asarray(b["input_ids"]).astype(np.int64), clip, n_new, (), pick=pick):
            pass
    torch.cuda.synchronize()
    assert m.last_decode_path == ("graph" if graph else "loop")
    assert len(generated) == n_new and len(hiddens) == n_new
    return list(generated), [h.reshape(-1).float().cpu() for h in hiddens[1:]]


def _count_calls(monkeypatch, name):
    n = [0]
    orig = getattr(ops, name)

    def counted(*a, **kw):
        n[0] += 1
        return orig(*a, **kw)
    monkeypatch.setattr(ops, name, counted)
    return n


# ---------------------------------------------------------------- what differs between the modes
def _snap_rows_w8(w):
    """Every row -> c * 2^e with integer |c| <= 127 and the row's largest entry at +-127: what the quantiser reproduces exactly
    (tests/test_gpu_w8_gemv.py), so code * scale IS the bf16 weight."""
    absmax = w.abs().amax(-1, keepdim=True).clamp_min(2.0 ** -20)
    step = torch.exp2(torch.ceil(torch.log2(absmax / 127.0)))
    c = torch.round(w / step).clamp_(-127, 127)
    at = w.abs().argmax(-1, keepdim=True)
    c.scatter_(-1, at, 127.0 * torch.sign(w.gather(-1, at)))
    return c * step


def _snap_blocks_nf4(w):
    """Every block of 64 of every row -> bf16(NF4[c]) * 2^e with the block's largest entry at +-1 * 2^e: what the quantiser reproduces
    exactly (tests/test_gpu_w4_gemv.py), so table[code] * absmax IS the bf16 weight."""
    w = w.unflatten(-1, (-1, R.BLOCK))
    table = R.NF4_BF16.to(w.device)
    absmax = w.abs().amax(-1, keepdim=True).clamp_min(2.0 ** -20)
    step = torch.exp2(torch.ceil(torch.log2(absmax)))
    c = ((w / step).unsqueeze(-1) - table).abs().argmin(-1)
    at = w.abs().argmax(-1, keepdim=True)
    c.scatter_(-1, at, torch.where(w.gather(-1, at) < 0, 0, 15))
    return (table[c] * step).flatten(-2)


def _dequant_w8(codes, scale):
    return (codes.float() * scale.unsqueeze(-1)).cpu()


def _compare_w8(m, deq, monkeypatch):
    """The comparison run of the 8-bit mode: a model whose decoder projections were replaced by bf16(code * scale) BEFORE the prefill.  That
    carries one extra bf16 rounding of the weights (code * scale has up to 7 + 24 significant bits), and the 8-bit run's PREFILL used the
    original bf16 weights where this model's uses the dequantised ones; both are far below the bound."""
    llm = m.model.llm
    for lw, dq in zip(llm.layers, deq):
        for k in KEYS:
            lw[k].copy_(dq[k])
    llm.refresh_fused_qkv()
    ops.PARAM_EPOCH += 1


def _compare_w4(m, deq, monkeypatch):
    """The comparison run of the 4-bit mode: its DECODE steps read bf16(dequant) in place of the decoder projections.  The 4-bit mode leaves
    the prefill on the original bf16 weights, so the comparison run does too: its weights are swapped between its prefill and its first step.
    (NF4 moves a weight by up to ~10 % of its block's absmax: a comparison run that also PREFILLED on the dequantised weights decodes against
    another KV cache and lies 0.096 of the max entry away, dense — measured; that is the quantisation error of the prompt, not of the step
    under test.)  What is left is one extra bf16 rounding of the weights (table * absmax has up to 8 + 24 significant bits)."""
    llm, prefill = m.model.llm, m._prefill

    def prefill_then_swap(*a, **kw):
        out = prefill(*a, **kw)
        for lw, dq in zip(llm.layers, deq):
            for k in KEYS:
                lw[k].copy_(dq[k])
        return out
    monkeypatch.setattr(m, "_prefill", prefill_then_swap)


# per mode: the ops pair and the other mode's GEMV, the dimension multiple, the grid snap, the dequantiser (-> fp32 on the host) and the
# builder of the comparison run of test_mode_is_really_on_with_random_weights
_Mode = collections.namedtuple("_Mode", "quantizer gemv other_gemv multiple snap dequant compare")
MODES = {8: _Mode("quantize_rows_w8", "gemv_w8", "gemv_w4", 16, _snap_rows_w8, _dequant_w8, _compare_w8),
         4: _Mode("quantize_blocks_nf4", "gemv_w4", "gemv_w8", 64, _snap_blocks_nf4, R.dequant_ref, _compare_w4)}


def _enable(m, bits, on):
    return getattr(m, f"enable_decode_{bits}bit")(on)


def _is_on(m, bits):
    return getattr(m, f"decode_{bits}bit")


def _snap_to_grid(m, bits):
    llm = m.model.llm
    for lw in llm.layers:
        for k in KEYS:
            snapped = MODES[bits].snap(lw[k].float())
            lw[k].copy_(snapped.to(torch.bfloat16))
            assert torch.equal(lw[k].float(), snapped)
    llm.refresh_fused_qkv()
    ops.PARAM_EPOCH += 1


# ---------------------------------------------------------------- the tests, each under both modes
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bits", BITS)
def test_teacher_forced_hidden_states_match_bf16_on_grid_weights(dev, bits, kind, monkeypatch):
    """The tokens of a 16-token bf16 greedy run, fed to the quantised run through a scripted pick: every per-step hidden state within
    2^-5 * max|entry| of the bf16 run's, in the captured step and in the loop.  Top-1: a near-tied gate may send one step to the other
    expert, so the bound may fail on at most one of the 15 compared steps; dense: on none."""
    mode = MODES[bits]
    cfg, m = _tiny(dev, kind)
    _snap_to_grid(m, bits)
    b, clip, _ = _inputs(cfg, dev)
    calls, other = _count_calls(monkeypatch, mode.gemv), _count_calls(monkeypatch, mode.other_gemv)
    for graph in (True, False):
        _enable(m, bits, False)
        toks, hb = _run(m, b, clip, graph)
        assert calls[0] == 0 and not _is_on(m, bits)
        pick = _ScriptedPick(toks, dev)
        toks_b, hb2 = _run(m, b, clip, graph, pick=pick)                 # (the scripted pick itself: the bf16 run again, bit for bit)
        assert toks_b == toks and all(torch.equal(x, y) for x, y in zip(hb, hb2))
        _enable(m, bits, True)
        for lw, q in zip(m.model.llm.layers, m.model.llm.decode_weights.copies):     # on the grid the copies ARE the weights
            assert all(torch.equal(mode.dequant(*q[k]), lw[k].float().cpu()) for k in KEYS)
        toks_q, hq = _run(m, b, clip, graph, pick=pick)
        assert _is_on(m, bits) and calls[0] > 0 and other[0] == 0 and toks_q == toks and len(hq) == N_NEW - 1
        rel = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(hq, hb)]
        print(bits, kind, "graph" if graph else "loop", "max |hq - hbf16| / max|hbf16| per step:", " ".join(f"{r:.4f}" for r in rel))
        assert sum(r > BOUND for r in rel) <= (1 if kind == "top1" else 0), rel
        calls[0] = 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bits", BITS)
def test_mode_is_really_on_with_random_weights(dev, bits, kind, monkeypatch):
    """Off-grid weights: the quantised run's first decode-step hidden state differs from the bf16 run's, and equals — within the same bound —
    the mode's comparison run on bf16(dequantised weights) (MODES[bits].compare: what each builds, and why they differ)."""
    mode = MODES[bits]
    cfg, m = _tiny(dev, kind)
    b, clip, _ = _inputs(cfg, dev)
    toks, _ = _run(m, b, clip, True, n_new=4)
    pick = _ScriptedPick(toks, dev)
    _, hb = _run(m, b, clip, True, pick=pick, n_new=4)
    _enable(m, bits, True)
    _, h = _run(m, b, clip, True, pick=pick, n_new=4)
    assert not torch.equal(h[0], hb[0])
    _enable(m, bits, False)
    quantize = getattr(ops, mode.quantizer)
    deq = [{k: mode.dequant(*quantize(lw[k])).to(torch.bfloat16).to(dev) for k in KEYS} for lw in m.model.llm.layers]
    mode.compare(m, deq, monkeypatch)
    _, hq = _run(m, b, clip, True, pick=pick, n_new=4)
    rel_q = float((h[0] - hq[0]).abs().max() / hq[0].abs().max())
    rel_b = float((h[0] - hb[0]).abs().max() / hb[0].abs().max())
    print(bits, kind, f"step 1: |h - h(dequantised bf16)| = {rel_q:.5f}, |h - h(bf16)| = {rel_b:.5f} (of the max entry)")
    assert rel_q <= BOUND


def every_decoding_entry_point_runs(dev, bits, kind, monkeypatch):
    """The body of the entry-point test of either mode (the 8-bit one keeps its name and place in tests/test_gpu_w8_decode.py)."""
    cfg, m = _tiny(dev, kind)
    b, clip, sam = _inputs(cfg, dev)
    n_in = b["input_ids"].shape[1]
    _enable(m, bits, True)
    calls, other = _count_calls(monkeypatch, MODES[bits].gemv), _count_calls(monkeypatch, MODES[bits].other_gemv)
    for graph in (True, False):
        m.decode_with_graph = graph
        path = "graph" if graph else "loop"
        seen = calls[0]
        out = m.generate(b["input_ids"], images=clip, max_new_tokens=6, eos_token_id=-1)
        assert out.shape == (1, n_in + 6) and m.last_decode_path == path and calls[0] > seen
        seen = calls[0]
        out = m.generate_sample(b["input_ids"], images=clip, max_new_tokens=6, eos_token_id=-1, temperature=0.8, sample_seed=5)
        assert out.shape == (1, n_in + 6) and m.last_decode_path == path and calls[0] > seen
        again = m.generate_sample(b["input_ids"], images=clip, max_new_tokens=6, eos_token_id=-1, temperature=0.8, sample_seed=5)
        assert torch.equal(out, again), "one seed, one answer"
        seen = calls[0]
        out = m.generate_beam(b["input_ids"], images=clip, max_new_tokens=6, eos_token_id=-1, num_beams=3)      # M = 3 rows per step
        assert out.shape == (1, n_in + 6) and m.last_decode_path == path and calls[0] > seen
        seen = calls[0]
        ys = list(m.generate_stream(b["input_ids"], clip, temperature=0.0, max_new_tokens=6, eos_token_id=-1))
        assert len(ys[-1][0]) == 6 and m.last_decode_path == path and calls[0] > seen
        greedy = m.generate(b["input_ids"], images=clip, max_new_tokens=6, eos_token_id=-1)[0, n_in:].tolist()
        assert ys[-1][0] == greedy
    ids, masks = m.evaluate(clip, sam, b["input_ids"], b["resize_list"], b["label_list"], max_new_tokens=6, eos_token_id=-1)
    assert ids.shape == (1, n_in + 6) and len(masks) == 1 and masks[0].dim() == 3 and _is_on(m, bits)
    assert other[0] == 0 and not any(_is_on(m, o) for o in BITS if o != bits)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bits", BITS[1:])
def test_every_decoding_entry_point_runs_in_the_quantised_mode(dev, bits, kind, monkeypatch):
    every_decoding_entry_point_runs(dev, bits, kind, monkeypatch)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bits", BITS)
def test_off_means_off(dev, bits, kind):
    cfg, m = _tiny(dev, kind)
    b, clip, _ = _inputs(cfg, dev)
    for graph in (True, False):
        before = _run(m, b, clip, graph)
        _enable(m, bits, True)
        _run(m, b, clip, graph, n_new=4)
        _enable(m, bits, False)
        assert not _is_on(m, bits) and m.model.llm.decode_weights is None          # (copies and epoch: one state)
        after = _run(m, b, clip, graph)
        assert after[0] == before[0] and all(torch.equal(x, y) for x, y in zip(after[1], before[1]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bits", BITS)
def test_a_parameter_write_requantises_before_the_next_decode(dev, bits, kind):
    """ops.PARAM_EPOCH moves (an optimizer step, a checkpoint load): the decode prologue re-quantises, so the next decode equals that of a
    freshly enabled model — and not the decode before the write."""
    cfg, m = _tiny(dev, kind)
    b, clip, _ = _inputs(cfg, dev)
    _enable(m, bits, True)
    old = _run(m, b, clip, True)
    for lw in m.model.llm.layers:
        lw["o"].mul_(0.5)
        lw["down"].mul_(-1.0)
    ops.PARAM_EPOCH += 1
    assert m.model.llm.decode_weights.epoch != ops.PARAM_EPOCH
    new = _run(m, b, clip, True)
    assert m.model.llm.decode_weights.epoch == ops.PARAM_EPOCH and _is_on(m, bits)
    _enable(m, bits, False)
    _enable(m, bits, True)
    fresh = _run(m, b, clip, True)
    assert new[0] == fresh[0] and all(torch.equal(x, y) for x, y in zip(new[1], fresh[1]))
    assert not all(torch.equal(x, y) for x, y in zip(new[1], old[1]))


@pytest.mark.parametrize("bits", BITS)
def test_refusals_leave_the_model_decoding_in_bf16(dev, bits, monkeypatch):
    from medplib_amd.model.llama import LlamaStack
    calls = _count_calls(monkeypatch, MODES[bits].gemv)

    def refused(m, cfg, match):
        b, clip, _ = _inputs(cfg, dev)
        before = m.generate(b["input_ids"], images=clip, max_new_tokens=4, eos_token_id=-1)
        with pytest.raises(NotImplementedError, match=match):
            _enable(m, bits, True)
        assert not _is_on(m, bits)
        assert torch.equal(m.generate(b["input_ids"], images=clip, max_new_tokens=4, eos_token_id=-1), before) and calls[0] == 0

    cfg, m = _tiny(dev, "top2")
    refused(m, cfg, "top-2")
    cfg, m = _tiny(dev, "top1", use_residual=True)
    refused(m, cfg, "use_residual")
    cfg, m = _tiny(dev, "top1")
    m.enable_lora(lora_r=8, lora_alpha=16, lora_target_modules="gate_proj,up_proj,down_proj")
    refused(m.eval(), cfg, "merge_and_unload")
    # adapters attached AFTER the mode was enabled: the decode prologue refuses, before anything is decoded
    cfg, m = _tiny(dev, "dense")
    _enable(m, bits, True)
    m.enable_lora(lora_r=8, lora_alpha=16, lora_target_modules="gate_proj,up_proj,down_proj")
    b, clip, _ = _inputs(cfg, dev)
    with pytest.raises(NotImplementedError, match="merge_and_unload"):
        m.eval().generate(b["input_ids"], images=clip, max_new_tokens=4, eos_token_id=-1)
    # a K that is no multiple of 16 / 64 (the stack alone: no decode launch takes such a config either way)
    llm = LlamaStack(MedPLIBConfig.tiny(moe_enable=False, intermediate_size=328), dev)
    with pytest.raises(NotImplementedError, match=f"multiples of {MODES[bits].multiple}"):
        llm.quantize_decode_weights(bits)
    assert llm.decode_weights is None and calls[0] == 0


@pytest.mark.parametrize("kind", KINDS)
def test_the_two_modes_are_exclusive(dev, kind, monkeypatch):
    cfg, m = _tiny(dev, kind)
    b, clip, _ = _inputs(cfg, dev)
    llm = m.model.llm
    calls4, calls8 = _count_calls(monkeypatch, "gemv_w4"), _count_calls(monkeypatch, "gemv_w8")
    m.enable_decode_8bit(True)
    m.enable_decode_4bit(True)
    assert llm.decode_weights.mode.bits == 4 and m.decode_4bit and not m.decode_8bit
    four = m.generate(b["input_ids"], images=clip, max_new_tokens=4, eos_token_id=-1)
    assert calls4[0] > 0 and calls8[0] == 0
    m.enable_decode_8bit(True)
    assert llm.decode_weights.mode.bits == 8 and m.decode_8bit and not m.decode_4bit
    seen = calls4[0]
    m.generate(b["input_ids"], images=clip, max_new_tokens=4, eos_token_id=-1)
    assert calls8[0] > 0 and calls4[0] == seen
    m.enable_decode_4bit(True)
    assert torch.equal(m.generate(b["input_ids"], images=clip, max_new_tokens=4, eos_token_id=-1), four)
