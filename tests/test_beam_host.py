"""CPU: the two beam-search entry points (mp_beam_topk_f32, mp_kv_permute_rows_bf16) are declared in include/medplib_hip.h, exported by the
library and refuse bad arguments before any launch; the ops wrappers refuse CPU tensors; the seeded kernel cases keep their float64 gap;
and the host scorer (medplib_amd.beam.BeamScorer), driven by the float64 step rule on a tiny HF Llama's own logits, gives the tokens of
transformers' generate(num_beams=)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from beam_cases import GAP, all_cases, beam_step_rule, case_rule, needs_round32
from medplib_amd import _lib
from medplib_amd.beam import BeamScorer

TOPK, PERMUTE = "mp_beam_topk_f32", "mp_kv_permute_rows_bf16"


def test_header_declares_and_library_exports_both_entry_points():
    protos = _lib.parse_header()
    assert protos[TOPK][0] == "int" and protos[PERMUTE][0] == "int"
    assert [n for _, n in protos[TOPK][1]] == ["logits", "ld", "nb", "cols", "beam_scores", "eos_id", "cand_score", "cand_index", "next_scores",
                                               "next_tokens", "next_parent", "err", "stream"]
    assert [t for t, _ in protos[TOPK][1]] == ["const float*", "int64_t", "int", "int", "const float*", "int", "float*", "int*", "float*",
                                               "int64_t*", "int*", "int*", "hipStream_t"]
    assert [n for _, n in protos[PERMUTE][1]] == ["tensors", "n", "parent", "nb", "batch_stride", "row_elems", "lo", "hi_dev", "cache_rows", "err",
                                                  "stream"]
    assert [t for t, _ in protos[PERMUTE][1]] == ["const void*", "int", "const int*", "int", "int64_t", "int64_t", "int", "const int*", "int", "int*",
                                                  "hipStream_t"]
    header = open(_lib.HEADER_PATH).read()
    assert "#define MP_POS_ERR_BEAM 4" in header and "#define MP_POS_ERR_TABLE 1" in header and "#define MP_POS_ERR_CACHE 2" in header
    if not os.path.exists(_lib.LIB_PATH):
        from medplib_amd import build
        build.build(verbose=False)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(dll, TOPK) and hasattr(dll, PERMUTE)


def test_both_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    topk, permute = L.raw(TOPK), L.raw(PERMUTE)
    one = ctypes.c_void_p(16)                                     # (never dereferenced: a refused call launches nothing)
    ok = dict(ld=32000, nb=4, cols=32000)
    for change in (dict(nb=0), dict(nb=9), dict(nb=-1), dict(cols=1), dict(cols=65537, ld=65537), dict(ld=31999), dict(ld=-1)):
        a = dict(ok, **change)
        for ptr in (None, one):                                   # the shape is refused first, null operands or not
            assert topk(ptr, a["ld"], a["nb"], a["cols"], ptr, 2, ptr, ptr, ptr, ptr, ptr, ptr, None) == -1, change
            assert TOPK in L.last_error(), change
    assert topk(None, 32000, 4, 32000, None, 2, None, None, None, None, None, None, None) == -5
    assert TOPK in L.last_error() and "null operand" in L.last_error()
    for hole in range(8):                                         # any single null operand
        ptrs = [None if i == hole else one for i in range(8)]
        assert topk(ptrs[0], 0, 4, 32000, ptrs[1], -1, *ptrs[2:], None) == -5, hole
    ok = dict(n=64, nb=4, stride=40 * 4096, row=4096, lo=7, rows=40)
    bad = (dict(nb=0), dict(nb=9), dict(row=4100), dict(row=0), dict(row=-8), dict(n=-1), dict(rows=0), dict(lo=-1), dict(stride=40 * 4096 - 8),
           dict(stride=40 * 4096 + 4))
    for change in bad:
        a = dict(ok, **change)
        for ptr in (None, one):
            assert permute(ptr, a["n"], ptr, a["nb"], a["stride"], a["row"], a["lo"], ptr, a["rows"], ptr, None) == -1, change
            assert PERMUTE in L.last_error(), change
    a = ok
    assert permute(None, a["n"], None, a["nb"], a["stride"], a["row"], a["lo"], None, a["rows"], None, None) == -5
    assert PERMUTE in L.last_error() and "null operand" in L.last_error()
    assert permute(None, 0, None, a["nb"], a["stride"], a["row"], a["lo"], None, a["rows"], None, None) == 0      # no tensors: nothing to do


def test_wrappers_refuse_cpu_tensors():
    from medplib_amd import ops
    f, i, l = (lambda n: torch.zeros(n)), (lambda n: torch.zeros(n, dtype=torch.int32)), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.beam_topk(torch.zeros(2, 8), f(2), -1, f(4), i(4), f(2), l, i(2), i(1))
    kv = torch.zeros(2, 4, 8, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.kv_permute_rows(torch.zeros(1, dtype=torch.int64), kv, i(2), 0, i(1), i(1))
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.kv_permute_table([kv])


def test_every_kernel_case_keeps_its_gap():
    """The precondition the GPU test asserts again, checked here for every seeded case: adjacently ranked candidates (ranks 0 .. 2 nb) are
    GAP apart in float64, all 2 nb exist, and the ranked scores stay below 2^7 — except where first-step scores reach into the -1e9 beams
    (needs_round32), which fp32 cannot tell apart and the rule ranks as fp32 does."""
    n = 0
    for nb, cols, ld, scores, seed in all_cases():
        r = case_rule(nb, cols, ld, scores, seed)
        assert r["gap"] >= GAP and not r["unfilled"], (nb, cols, ld, scores, seed, r["gap"])
        assert needs_round32(nb, cols, scores) or np.abs(r["cand_score"]).max() < 128, (nb, cols, ld, scores)
        n += 1
    assert n == 4 * 8 * 3 * 2


def test_step_rule_ties_eos_and_nan():
    l = np.array([[1.0, 1.0, 0.0, np.nan], [1.0, 1.0, 0.0, 0.5]])
    r = beam_step_rule(l, [0.0, 0.0], eos=1)
    z0, z1 = np.log(2 * np.e + 1), np.log(2 * np.e + 1 + np.exp(0.5))
    assert r["cand_index"].tolist() == [0, 1, 4, 5]               # beam 0's pair leads (a smaller Z), ties by flat index; the NaN never ranks
    assert np.allclose(r["cand_score"], [1 - z0, 1 - z0, 1 - z1, 1 - z1]) and r["gap"] == 0.0
    assert r["next_tokens"].tolist() == [0, 0] and r["next_parent"].tolist() == [0, 1]
    few = beam_step_rule(np.array([[0.0, np.nan, np.nan]]), [0.0, -1.0], eos=-1)
    assert few["unfilled"] and few["cand_index"].tolist() == [0, 3, -1, -1] and few["cand_score"][2] == -np.inf


# ---------------------------------------------------------------------------------------------------------------- the scorer
def _cands(*triples):
    return [tuple(t) for t in triples]


def test_early_stopping_true_stops_at_the_first_step_with_nb_hypotheses():
    eos = 9
    for early, stops_at in ((True, 1), (False, None)):
        sc = BeamScorer(2, length_penalty=1.0, early_stopping=early, eos_token_id=eos, length_base=4, max_new_tokens=6)
        assert not sc.step(_cands((-0.5, 0, 3), (-0.6, 0, 4), (-9.0, 0, 5), (-9.5, 0, 6)))
        # both top ranks end on eos: two hypotheses at once.  Their scores (-2 / 5, -2.2 / 5) are far below what the running beams can still
        # reach (-0.7 / 5), so only early stopping ends the search here
        done = sc.step(_cands((-2.0, 0, eos), (-2.2, 1, eos), (-0.7, 0, 1), (-0.8, 1, 2)))
        assert done == (stops_at == 1) and len(sc.hyps) == 2
        if early:
            toks, score = sc.finalize()
            assert toks == [3, eos] and score == -2.0 / 5
        else:                                                      # early_stopping=False: done once no running beam can beat the worst one
            assert not sc.step(_cands((-0.75, 0, 1), (-0.85, 1, 2), (-20.0, 0, 5), (-21.0, 0, 6)))           # -0.75 / 6 > -2.2 / 5
            assert sc.step(_cands((-4.0, 0, 1), (-4.1, 1, 2), (-20.0, 0, 5), (-21.0, 0, 6)))                 # -4.0 / 7 < -2.2 / 5
            toks, score = sc.finalize()
            assert toks == [3, eos] and score == -2.0 / 5 and sc.steps == 4


def test_an_eos_below_rank_nb_is_ignored_and_the_best_running_beam_wins_at_the_end():
    sc = BeamScorer(2, length_penalty=0.0, eos_token_id=9, length_base=3, max_new_tokens=2)
    assert not sc.step(_cands((-0.1, 0, 1), (-0.2, 0, 2), (-0.3, 0, 9), (-0.4, 0, 3)))        # eos at rank 2 = nb: no hypothesis
    assert sc.hyps == [] and sc.beams == [[1], [2]]
    assert not sc.step(_cands((-0.5, 1, 4), (-0.6, 0, 9), (-0.7, 0, 5), (-0.8, 1, 6)))        # eos at rank 1 < nb: beam [1] ends
    assert sc.hyps == [(-0.6, [1])] and sc.beams == [[2, 4], [1, 5]]
    toks, score = sc.finalize()
    assert toks == [2, 4] and score == -0.5                       # full length: no eos appended


def test_length_base_enters_exactly_as_stated():
    """Two hypotheses, one generated token against five: sum / (length_base + n) ** lp.  With the prompt counted (length_base = 20) the short
    one wins, -1.0 / 21 > -1.3 / 25; with length_base = 0 the long one does, -1.3 / 5 > -1.0 / 1."""
    def run(base):
        sc = BeamScorer(1, length_penalty=1.0, eos_token_id=9, length_base=base, max_new_tokens=8)
        sc._add([5], -1.0)
        short = sc.hyps[0][0]
        sc.num_beams = 2                                           # (room for both, to read both scores)
        sc._add([1, 2, 3, 4, 6], -1.3)
        return short, sc.hyps[1][0], sc
    short, long_, sc = run(20)
    assert short == -1.0 / 21 and long_ == -1.3 / 25 and short > long_ and sc.length(5) == 25
    short, long_, sc = run(0)
    assert short == -1.0 / 1 and long_ == -1.3 / 5 and long_ > short and sc.length(5) == 5
    # and in the done test: cur_len = length_base + t
    sc = BeamScorer(1, length_penalty=1.0, eos_token_id=9, length_base=10, max_new_tokens=8)
    sc._add([5], -1.1)
    assert sc.worst_score == -1.1 / 11
    assert sc._is_done(-1.2, 1) and not sc._is_done(-1.0, 1)     # -0.1 >= -1.2 / 11; -0.1 < -1.0 / 11


def _hf_tiny():
    try:
        from transformers import LlamaConfig, LlamaForCausalLM
    except Exception as e:                                         # noqa: BLE001
        pytest.skip(f"transformers' generate does not import: {e}")
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=320, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                      max_position_embeddings=64)
    return LlamaForCausalLM(cfg).eval()


_HF = {}


def _search(model, prompt, nb, eos, n_new):
    """The scorer driven by beam_step_rule on the model's own step logits (the beams re-run without a cache)
    -> (tokens, stopped before n_new)."""
    sc = BeamScorer(nb, length_penalty=0.0, early_stopping=False, eos_token_id=eos, length_base=prompt.shape[1], max_new_tokens=n_new)
    scores = np.array([0.0] + [-1e9] * (nb - 1))
    for t in range(n_new):
        ids = torch.cat([prompt.expand(nb, -1), torch.tensor(sc.beams, dtype=torch.int64).view(nb, t)], 1)
        with torch.no_grad():
            logits = model(ids).logits[:, -1].double().numpy()
        r = beam_step_rule(logits, scores, eos)
        done = sc.step([(float(s), int(i) // 320, int(i) % 320) for s, i in zip(r["cand_score"], r["cand_index"])])
        assert [b[-1] for b in sc.beams] == r["next_tokens"].tolist() and sc.scores == r["next_scores"].tolist()
        scores = r["next_scores"]
        if done:
            break
    return sc.finalize()[0], sc.done


@pytest.mark.parametrize("nb", (2, 3, 4, 8))
def test_scorer_gives_the_tokens_of_transformers_generate(nb):
    """length_penalty = 0 cancels the length convention (where 4.31 and the installed release differ).  eos ids 7, 202, 85, 45 and prompt
    seeds 0..2; and, so that hypotheses do finish on this random model, per seed an eos taken from the answer of the search without one."""
    if "m" not in _HF:
        _HF["m"] = _hf_tiny()
    model, n_new, hit_eos, early = _HF["m"], 12, 0, 0

    def hf(prompt, eos):
        with torch.no_grad():
            return model.generate(prompt, num_beams=nb, length_penalty=0.0, early_stopping=False, max_new_tokens=n_new, do_sample=False,
                                  eos_token_id=eos, pad_token_id=eos, num_return_sequences=1)[0, prompt.shape[1]:].tolist()

    for seed in range(3):
        prompt = torch.randint(0, 320, (1, 9), generator=torch.Generator().manual_seed(seed))
        free = _search(model, prompt, nb, -1, n_new)[0]
        for eos in (7, 202, 85, 45, free[3], free[8]):
            ref = hf(prompt, eos)
            toks, stopped = _search(model, prompt, nb, eos, n_new)
            hit_eos += toks[-1] == eos
            early += stopped
            assert toks + [eos] * (len(ref) - len(toks)) == ref, (nb, eos, seed, toks, ref)
    assert hit_eos >= 3 and early >= 1, (hit_eos, early)
