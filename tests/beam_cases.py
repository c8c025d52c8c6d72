"""Helpers of the beam-search tests (no test in here): the float64 statement of one selection step (mp_beam_topk_f32's contract, HF 4.31's
log_softmax + beam_scores -> top 2 nb -> BeamSearchScorer.process) and the seeded cases the kernel is held to."""
import numpy as np
import torch

NBS = (1, 2, 3, 8)
COLS = (2, 63, 515, 4099, 32011, 32768, 32769, 65536)
LDS = ("cols", "cols+3", "zero")            # row stride: cols, cols + 3 (rows off 16 bytes), 0 (every beam reads one row)
SCORES = ("first", "spread")                # HF's first-step [0, -1e9, ...]; running scores spread over a few nats
GAP = 1e-3                                  # float64 gap asked between adjacently ranked candidates: over a hundred fp32 ulps below 2^7


def beam_step_rule(logits64, scores64, eos, round32=False):
    """One selection step in float64.  logits64 [nb, cols] (or [1, cols]: every beam reads that row), scores64 [nb].
    value v(b, c) = (l - m_b) - log sum exp(l - m_b) + scores[b]; NaN columns are left out of m_b and the sum and are never candidates; a row
    whose maximum is not finite has none.  Ranking: value descending, then flat index b * cols + c ascending; the best 2 nb are the candidates
    (unfilled: index -1, score -inf).  Selection: in rank order, skipping tokens equal to eos, the first nb.
    round32: the values are rounded to fp32 before they are ranked (values that fp32 cannot tell apart tie, as they do on the device).
    -> dict(cand_score, cand_index, next_scores, next_tokens, next_parent, gap, unfilled); gap = the smallest float64 difference between
    adjacently ranked candidates among ranks 0 .. 2 nb (rank 2 nb = the first one rejected); pairs that tie under round32 do not count."""
    scores64 = np.asarray(scores64, dtype=np.float64)
    nb = scores64.shape[0]
    l = np.asarray(logits64, dtype=np.float64)
    if l.shape[0] == 1 and nb > 1:
        l = np.broadcast_to(l, (nb, l.shape[1]))
    cols = l.shape[1]
    v = np.full((nb, cols), np.nan)
    with np.errstate(all="ignore"):
        for b in range(nb):
            ok = ~np.isnan(l[b])
            if not ok.any():
                continue
            m = l[b][ok].max()
            if not np.isfinite(m):
                continue
            z = np.exp(l[b][ok] - m).sum()
            v[b] = (l[b] - m) - np.log(z) + scores64[b]
    flat = np.flatnonzero(~np.isnan(v.reshape(-1)))
    vals = v.reshape(-1)[flat]
    key = vals.astype(np.float32).astype(np.float64) if round32 else vals
    order = np.lexsort((flat, -key))[:2 * nb + 1]
    r_idx, r_val, r_key = flat[order], vals[order], key[order]
    gap = np.inf
    with np.errstate(all="ignore"):
        for a in range(len(order) - 1):
            if round32 and r_key[a] == r_key[a + 1]:
                continue
            g = r_val[a] - r_val[a + 1]
            gap = min(gap, 0.0 if np.isnan(g) else g)
    n = min(2 * nb, len(order))
    cand_score = np.full(2 * nb, -np.inf)
    cand_index = np.full(2 * nb, -1, dtype=np.int64)
    cand_score[:n], cand_index[:n] = r_val[:n], r_idx[:n]
    nxt = [(cand_score[r], cand_index[r] % cols, cand_index[r] // cols) for r in range(n) if cand_index[r] % cols != eos][:nb]
    nxt += [(-np.inf, 0, 0)] * (nb - len(nxt))
    return {"cand_score": cand_score, "cand_index": cand_index, "next_scores": np.array([x[0] for x in nxt]),
            "next_tokens": np.array([x[1] for x in nxt], dtype=np.int64), "next_parent": np.array([x[2] for x in nxt], dtype=np.int64),
            "gap": gap, "unfilled": n < 2 * nb}


def needs_round32(nb, cols, scores):
    """First-step scores rank candidates of the -1e9 beams only when beam 0's row is shorter than the 2 nb + 1 ranked ones: cols = 2 with
    nb >= 2.  fp32 cannot tell those values apart (an ulp of 1e9 is 64), on the device as in HF, so these cases are ranked on the fp32-rounded
    float64 values; every other case is ranked in float64 and its ranked scores stay below 2^7."""
    return scores == "first" and cols < 2 * nb + 1 and nb > 1


def beam_case(nb, cols, ld, scores, seed):
    """-> (logits fp32 [rows, ld or cols] backing tensor, logits view [nb or 1, cols], scores fp32 [nb]) of one seeded case."""
    g = torch.Generator().manual_seed(seed)
    rows = 1 if ld == "zero" else nb
    width = cols + 3 if ld == "cols+3" else cols
    back = torch.randn(rows, width, generator=g, dtype=torch.float32) * 3
    if scores == "first":
        s = torch.tensor([0.0] + [-1e9] * (nb - 1), dtype=torch.float32)
    else:
        s = -(torch.rand(nb, generator=g, dtype=torch.float32) * 6).sort().values
    return back, back[:, :cols], s


# cases whose default seed (0) leaves two ranked candidates closer than GAP: the first seed that does not (tests/test_beam_host.py checks all)
SEEDS = {(3, 515, "cols", "first"): 1, (3, 515, "cols+3", "first"): 1, (3, 515, "zero", "first"): 1, (8, 515, "cols", "first"): 1,
         (8, 515, "cols+3", "first"): 1, (8, 515, "cols+3", "spread"): 2, (8, 515, "zero", "first"): 1, (8, 4099, "cols", "first"): 1,
         (8, 4099, "cols+3", "first"): 1, (8, 4099, "zero", "first"): 1}


def all_cases():
    for nb in NBS:
        for cols in COLS:
            for ld in LDS:
                for scores in SCORES:
                    yield nb, cols, ld, scores, SEEDS.get((nb, cols, ld, scores), 0)


def case_rule(nb, cols, ld, scores, seed, eos=-1):
    _, view, s = beam_case(nb, cols, ld, scores, seed)
    return beam_step_rule(view.double().numpy(), s.double().numpy(), eos, round32=needs_round32(nb, cols, scores))
