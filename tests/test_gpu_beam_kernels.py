"""The two beam-search kernels against their statements: mp_beam_topk_f32 (ops.beam_topk) against the float64 step rule of
tests/beam_cases.py — exact candidates, order, selection and parents — and mp_kv_permute_rows_bf16 (ops.kv_permute_rows) against
index_select, bit for bit, canaries around everything it must not touch."""
import numpy as np
import pytest
import torch

from beam_cases import GAP, all_cases, beam_case, beam_step_rule, needs_round32
from medplib_amd import ops

pytestmark = pytest.mark.gpu


def _topk(dev, logits, scores, eos, nb=None, alias=False):
    """ops.beam_topk into fresh outputs -> dict of host arrays (+ err)."""
    nb = logits.shape[0] if nb is None else nb
    out = {"cand_score": torch.full((2 * nb,), 7.0, device=dev), "cand_index": torch.full((2 * nb,), -7, dtype=torch.int32, device=dev),
           "next_scores": scores if alias else torch.full((nb,), 7.0, device=dev),
           "next_tokens": torch.full((nb,), -7, dtype=torch.int64, device=dev), "next_parent": torch.full((nb,), -7, dtype=torch.int32, device=dev)}
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.beam_topk(logits, scores, eos, out["cand_score"], out["cand_index"], out["next_scores"], out["next_tokens"], out["next_parent"], err,
                  nb=nb)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["err"] = int(err[0])
    return res


def test_beam_topk_seeded_cases_equal_the_float64_rule(dev):
    """Every (nb, cols, ld, scores) case: the candidates' indices and order, the selected tokens and the parents equal the float64 rule's,
    with eos = -1 and with eos = the rule's best token (so that a candidate is skipped); cand_score within 1e-4 of float64 (where first-step
    scores reach into the -1e9 beams — cols = 2, nb >= 2 — fp32 holds -1e9 to 64 at best: those scores to one part in 2^23).  The case's own
    precondition is asserted first: a float64 gap of GAP between adjacently ranked candidates and ranked scores below 2^7."""
    n = 0
    for nb, cols, ld, scores, seed in all_cases():
        back, view, s = beam_case(nb, cols, ld, scores, seed)
        r32 = needs_round32(nb, cols, scores)
        l64, s64 = view.double().numpy(), s.double().numpy()
        logits = back.to(dev)[:, :cols]
        assert logits.stride(0) == (cols + 3 if ld == "cols+3" else cols)
        free = beam_step_rule(l64, s64, -1, round32=r32)
        for eos in (-1, int(free["next_tokens"][0])):
            ref = free if eos == -1 else beam_step_rule(l64, s64, eos, round32=r32)
            assert ref["gap"] >= GAP and not ref["unfilled"], (nb, cols, ld, scores, seed, ref["gap"])
            assert r32 or np.abs(ref["cand_score"]).max() < 128
            got = _topk(dev, logits, s.to(dev), eos, nb=nb)
            what = (nb, cols, ld, scores, seed, eos)
            assert got["err"] == 0, what
            assert got["cand_index"].tolist() == ref["cand_index"].tolist(), what
            assert got["next_tokens"].tolist() == ref["next_tokens"].tolist() and got["next_parent"].tolist() == ref["next_parent"].tolist(), what
            tol = np.maximum(1e-4, np.abs(ref["cand_score"]) * 2.0 ** -23) if r32 else 1e-4
            assert np.all(np.abs(got["cand_score"].astype(np.float64) - ref["cand_score"]) <= tol), what
            picked = [r for r in range(2 * nb) if ref["cand_index"][r] % cols != eos][:nb]
            assert got["next_scores"].tolist() == got["cand_score"][picked].tolist(), what       # the candidates' own bits
            n += 1
    assert n == 2 * 4 * 8 * 3 * 2


def _exact(dev, rows, scores, eos, **kw):
    """A crafted case whose values are exact in fp32 and float64 alike is held to the rule exactly, scores included where finite."""
    l = torch.tensor(rows, dtype=torch.float32)
    s = torch.tensor(scores, dtype=torch.float32)
    ref = beam_step_rule(l.double().numpy(), s.double().numpy(), eos)
    got = _topk(dev, l.to(dev), s.to(dev), eos, **kw)
    assert got["cand_index"].tolist() == ref["cand_index"].tolist(), (got, ref)
    assert got["next_tokens"].tolist() == ref["next_tokens"].tolist() and got["next_parent"].tolist() == ref["next_parent"].tolist()
    fin = np.isfinite(ref["cand_score"])
    assert np.allclose(got["cand_score"][fin], ref["cand_score"][fin], atol=1e-5, rtol=0)
    assert np.array_equal(got["cand_score"][~fin], ref["cand_score"][~fin])
    return got, ref


def test_beam_topk_ties_go_to_the_lower_flat_index(dev):
    # equal rows and equal scores: every value ties across the beams, and columns 1, 2 tie inside a row
    row = [0.0, 2.0, 2.0, -1.0, 1.0]
    got, _ = _exact(dev, [row, row, row], [-1.0, -1.0, -1.0], -1)
    assert got["cand_index"].tolist() == [1, 2, 6, 7, 11, 12] and got["next_parent"].tolist() == [0, 0, 1]
    assert len(set(got["cand_score"].tolist())) == 1
    # the same through ld = 0, and with a later beam ahead by its score
    got, _ = _exact(dev, [row], [-1.0, -1.0, -0.5], -1, nb=3)
    assert got["cand_index"].tolist() == [11, 12, 1, 2, 6, 7]
    # a wide row of one value: the first 2 nb columns of beam 0, then nothing of beam 1
    got, _ = _exact(dev, [[0.5] * 4099, [0.5] * 4099], [0.0, 0.0], -1)
    assert got["cand_index"].tolist() == [0, 1, 2, 3] and got["next_tokens"].tolist() == [0, 1]


def test_beam_topk_eos_at_ranks_below_and_above_nb(dev):
    # beam scores far enough apart that rank = (beam, column order): row values 3 > 2 > 1 > 0 at columns 4, 2, 0, 3
    row = [1.0, -5.0, 2.0, 0.0, 3.0, -6.0]
    nb = 3
    for eos, ranks in ((4, [0]), (2, [1]), (0, [2]), (3, [3]), (1, [4]), (5, [5]), (-1, [])):
        got, ref = _exact(dev, [row] * nb, [0.0, -20.0, -40.0], eos)
        assert [r for r in range(2 * nb) if got["cand_index"][r] % 6 == eos] == ranks
        assert eos not in got["next_tokens"].tolist() and got["err"] == 0
    # the most eos candidates there can be, nb: every beam's best column is eos and the beams tie, so ranks 0 .. nb-1 are all eos
    got, _ = _exact(dev, [row] * nb, [0.0, 0.0, 0.0], 4)
    assert (got["cand_index"][:nb] % 6).tolist() == [4] * nb and got["next_tokens"].tolist() == [2] * nb
    assert got["next_parent"].tolist() == [0, 1, 2]


def test_beam_topk_nan_and_inf_columns(dev):
    nan, inf = float("nan"), float("inf")
    # NaN columns are left out of the maximum and the sum and never rank; -inf columns rank last, by index
    got, _ = _exact(dev, [[nan, 1.0, -inf, 0.0, nan, -inf], [0.0, nan, nan, nan, nan, nan]], [0.0, -0.25], -1)
    assert got["cand_index"].tolist() == [6, 1, 3, 2] and got["err"] == 0 and got["cand_score"][3] == -inf
    assert got["cand_score"][0] == -0.25                                  # a row of one column: log-probability 0
    # fewer than 2 nb candidates: -1 / -inf entries, continuations that cannot be filled, and the error bit
    got, ref = _exact(dev, [[0.0, nan, nan], [nan, nan, nan]], [0.0, 0.0], -1)
    assert ref["unfilled"] and got["cand_index"].tolist() == [0, -1, -1, -1] and got["err"] == ops.POS_ERR_BEAM
    assert got["next_tokens"].tolist() == [0, 0] and got["next_parent"].tolist() == [0, 0] and got["next_scores"].tolist() == [0.0, -inf]
    # a row whose maximum is not finite has no candidates
    got, _ = _exact(dev, [[inf, 0.0, 1.0], [-inf, -inf, -inf], [0.0, 1.0, 0.0]], [0.0, 0.0, -3.0], -1)
    assert (got["cand_index"][:3] // 3).tolist() == [2, 2, 2] and got["cand_index"][3:].tolist() == [-1] * 3 and got["err"] == ops.POS_ERR_BEAM
    # NaN inside wide rows (register path and the re-read path): never chosen, whatever surrounds them
    for cols in (32011, 40000):
        g = torch.Generator().manual_seed(cols)
        l = torch.randn(2, cols, generator=g) * 3
        l[:, ::3] = nan
        ref = beam_step_rule(l.double().numpy(), [0.0, -0.5], -1)
        got = _topk(dev, l.to(dev), torch.tensor([0.0, -0.5], device=dev), -1)
        assert ref["gap"] >= GAP and got["cand_index"].tolist() == ref["cand_index"].tolist() and got["err"] == 0
        assert all(i % cols % 3 != 0 for i in got["cand_index"].tolist())


def test_beam_topk_aliased_scores_and_repeatable_bits(dev):
    nb, cols = 8, 32011
    _, view, s = beam_case(nb, cols, "cols", "spread", 0)
    logits = view.to(dev)
    first = _topk(dev, logits, s.to(dev), 5)
    running = s.to(dev)
    aliased = _topk(dev, logits, running, 5, alias=True)              # next_scores written over beam_scores
    assert torch.equal(running.cpu(), torch.from_numpy(first["next_scores"]))
    again = _topk(dev, logits, s.to(dev), 5)
    for k in ("cand_score", "cand_index", "next_scores", "next_tokens", "next_parent"):
        assert first[k].tobytes() == again[k].tobytes() == aliased[k].tobytes(), k
    # and inside a captured graph, replayed twice
    outs = {"cs": torch.zeros(2 * nb, device=dev), "ci": torch.zeros(2 * nb, dtype=torch.int32, device=dev), "ns": torch.zeros(nb, device=dev),
            "nt": torch.zeros(nb, dtype=torch.int64, device=dev), "np": torch.zeros(nb, dtype=torch.int32, device=dev)}
    err, s_dev = torch.zeros(1, dtype=torch.int32, device=dev), s.to(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            ops.beam_topk(logits, s_dev, 5, outs["cs"], outs["ci"], outs["ns"], outs["nt"], outs["np"], err)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for t in outs.values():
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k, name in (("cs", "cand_score"), ("ci", "cand_index"), ("ns", "next_scores"), ("nt", "next_tokens"), ("np", "next_parent")):
            assert outs[k].cpu().numpy().tobytes() == first[name].tobytes(), name


# ---------------------------------------------------------------------------------------------------------------- the cache re-order
ROWS = 40
PARENTS = {1: ([0],), 2: ([0, 1], [0, 0], [1, 0], [1, 1]), 5: ([0, 1, 2, 3, 4], [0, 0, 0, 0, 0], [1, 2, 3, 4, 0], [2, 2, 0, 1, 1]),
           8: ([0, 1, 2, 3, 4, 5, 6, 7], [0] * 8, [1, 2, 3, 4, 5, 6, 7, 0], [7, 7, 3, 3, 0, 1, 1, 5])}


def _pattern(shape, seed, dev):
    """Distinct-looking bf16 bit patterns (no NaN payload games: the copy is compared as int16 bits anyway)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-30000, 30000, shape, generator=g, dtype=torch.int16).to(dev).view(torch.bfloat16)


@pytest.mark.parametrize("nb", (1, 2, 5, 8))
def test_kv_permute_rows_equals_index_select(dev, nb):
    """n in {1, 4} tensors of a table of 4 + 1 allocated, row_elems in {8, 256, 4096}, 40 cache rows, every (lo, hi) and parent pattern:
    inside [lo, min(hi, 40)) the rows are index_select's, bit for bit; every other byte — positions outside, tensors not in the table, the
    guard rows around each tensor — keeps its pattern."""
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    for row_elems in (8, 256, 4096):
        shape = (nb, ROWS, row_elems)
        # each tensor sits inside a buffer with a guard row in front and behind
        bufs = [_pattern(((nb * ROWS + 2) * row_elems,), 100 * nb + i, dev) for i in range(5)]
        views = [b[row_elems:-row_elems].view(shape) for b in bufs]
        before = [b.clone() for b in bufs]
        for n in (1, 4):
            table, kept = ops.kv_permute_table(views[:n])
            assert table.numel() == n
            for lo, hi in ((0, 0), (7, 7), (7, 8), (7, 40), (0, 40), (7, 99)):
                hi_dev = torch.tensor([hi], dtype=torch.int32, device=dev)
                for parent in PARENTS[nb]:
                    for b, src in zip(bufs, before):
                        b.copy_(src)
                    par = torch.tensor(parent, dtype=torch.int32, device=dev)
                    ops.kv_permute_rows(table, views[0], par, lo, hi_dev, err)
                    top = min(hi, ROWS)
                    for i, (b, src) in enumerate(zip(bufs, before)):
                        want = src.clone()
                        if i < n and top > lo:
                            w = want[row_elems:-row_elems].view(shape)
                            w[:, lo:top] = src[row_elems:-row_elems].view(shape).index_select(0, par.long())[:, lo:top]
                        assert torch.equal(b.view(torch.int16), want.view(torch.int16)), (nb, row_elems, n, lo, hi, parent, i)
    assert int(err[0]) == 0


def test_kv_permute_rows_refuses_a_parent_out_of_range_on_the_device(dev):
    nb, row_elems = 5, 256
    t = _pattern((nb, ROWS, row_elems), 1, dev)
    before = t.clone()
    table, _ = ops.kv_permute_table([t])
    hi_dev = torch.tensor([ROWS], dtype=torch.int32, device=dev)
    for parent in ([1, 2, 3, 4, 5], [0, -1, 2, 3, 4]):
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        ops.kv_permute_rows(table, t, torch.tensor(parent, dtype=torch.int32, device=dev), 0, hi_dev, err)
        assert int(err[0]) == ops.POS_ERR_BEAM and torch.equal(t.view(torch.int16), before.view(torch.int16)), parent
    # the bit joins what the word already holds
    err = torch.tensor([2], dtype=torch.int32, device=dev)
    ops.kv_permute_rows(table, t, torch.tensor([9, 0, 0, 0, 0], dtype=torch.int32, device=dev), 0, hi_dev, err)
    assert int(err[0]) == 6


def test_kv_permute_rows_on_a_cache_of_the_stack_inside_a_graph(dev):
    """kv_permute_table over a {"k": [...], "v": [...]} cache, the bound read from a device counter a captured graph advances: each replay
    moves exactly the rows below the counter."""
    nb, L, H, D = 3, 2, 4, 16
    cache = {"k": [_pattern((nb, ROWS, H, D), 10 + i, dev) for i in range(L)], "v": [_pattern((nb, ROWS, H, D), 20 + i, dev) for i in range(L)]}
    want = [t.clone() for t in cache["k"] + cache["v"]]
    table, tensors = ops.kv_permute_table(cache)
    assert table.numel() == 2 * L and [t.data_ptr() for t in tensors] == table.cpu().tolist()
    counter = torch.tensor([12], dtype=torch.int32, device=dev)
    par = torch.tensor([2, 0, 0], dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            ops.kv_permute_rows(table, cache["k"][0], par, 10, counter[0:1], err)
            ops.advance_ints(counter, 1)
    torch.cuda.current_stream().wait_stream(side)
    for hi in (12, 13, 14):
        graph.replay()
        for w in want:
            w[:, 10:hi] = w.index_select(0, par.long())[:, 10:hi]
    torch.cuda.synchronize()
    assert int(counter[0]) == 15 and int(err[0]) == 0
    for t, w in zip(cache["k"] + cache["v"], want):
        assert torch.equal(t.view(torch.int16), w.view(torch.int16))
