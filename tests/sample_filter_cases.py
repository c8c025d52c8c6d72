"""Helper of the top-k / top-p sampling tests (not collected): the truncation rule of mp_sample_filtered_rows_f32 in float64 numpy, and the
rows the GPU tests run on.

The rule (include/medplib_hip.h; HF 4.31's Temperature -> TopK -> TopP warpers with their defaults): w_j = exp((l_j - max l) / T), NaN
columns weigh nothing and never survive.  Top-k (0 < k < cols): t_k = the k-th largest logit counting multiplicity, survivors l >= t_k (ties
all survive).  Top-p (p < 1) over the survivors: Z = sum of w, A(t) = sum of w over survivors with l <= t, kept iff A(l) / Z > 1 - p, the
group of the maximum always.  Equal logits share one fate."""
import numpy as np
import torch

from test_gpu_sample import _rows as _sample_rows

STDS = (0.5, 2.0, 4.0, 8.0)


def weights64(row, T):
    """float64 weights of the row: 1 at the maximum, 0 at NaN and -inf columns; all 0 for a row without a maximum above -inf."""
    l = np.asarray(row, dtype=np.float64)
    valid = ~np.isnan(l)
    if not valid.any() or l[valid].max() == -np.inf:
        return np.zeros_like(l)
    m = l[valid].max()
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(valid, np.exp((l - m) / T), 0.0)
    w[l == m] = 1.0
    return np.nan_to_num(w, nan=0.0)


class Row64:
    """The rule on one row at one temperature, prepared once: the non-NaN logits sorted ascending with their cumulative weights, so that
    every (k, p) costs a few binary searches."""

    def __init__(self, row, T):
        self.l = np.asarray(row, dtype=np.float64)
        self.cols = self.l.shape[0]
        self.valid = ~np.isnan(self.l)
        self.w = weights64(self.l, T)
        self.empty = not self.w.any()
        if not self.empty:
            idx = np.flatnonzero(self.valid)
            order = np.argsort(self.l[idx], kind="stable")
            self.ls, self.cw = self.l[idx][order], np.cumsum(self.w[idx][order])
            self.m = self.ls[-1]

    def t_k(self, k):
        """The k-th largest logit counting multiplicity (0 < k < cols), else the smallest one."""
        n = self.ls.size
        return float(self.ls[n - min(int(k), n)] if 0 < k < self.cols else self.ls[0])

    def mass(self, t, t_k):
        """A(t): the weight of the survivors (l >= t_k) with l <= t; t = m gives Z."""
        lo, hi = np.searchsorted(self.ls, t_k, side="left"), np.searchsorted(self.ls, t, side="right")
        return (self.cw[hi - 1] if hi > 0 else 0.0) - (self.cw[lo - 1] if lo > 0 else 0.0)

    def ratio(self, t, t_k):
        return self.mass(t, t_k) / self.mass(self.m, t_k)

    def below(self, t, t_k):
        """The next smaller distinct survivor logit under t, or None."""
        j = np.searchsorted(self.ls, t, side="left") - 1
        return float(self.ls[j]) if j >= 0 and self.ls[j] >= t_k else None

    def cut(self, k, p):
        """-> (the smallest kept logit, t_k)."""
        t_k = self.t_k(k)
        if p >= 1:
            return t_k, t_k
        lo = np.searchsorted(self.ls, t_k, side="left")
        base = self.cw[lo - 1] if lo > 0 else 0.0
        a = (self.cw[lo:] - base) / (self.cw[-1] - base)         # ascending; a group of equal logits is kept iff its LAST element passes,
        j = lo + np.searchsorted(a, 1.0 - p, side="right")       # and the first element that passes is the last of a group or inside a kept one
        return float(self.ls[j] if j < self.ls.size else self.m), t_k


def kept_rule(row, T, k, p):
    """-> (kept mask [cols] bool, A / Z per column (0 off the survivors), t_k).  A row with nothing to keep: (all False, zeros, +inf)."""
    r = Row64(row, T)
    if r.empty:
        return np.zeros(r.cols, bool), np.zeros(r.cols), np.inf
    cut, t_k = r.cut(k, p)
    surv = r.valid & (r.l >= t_k)
    lo = np.searchsorted(r.ls, t_k, side="left")
    base = r.cw[lo - 1] if lo > 0 else 0.0
    hi = np.searchsorted(r.ls, np.where(surv, r.l, r.m), side="right")
    ratio = np.where(surv, (r.cw[hi - 1] - base) / (r.cw[-1] - base), 0.0)
    kept = surv & ((ratio > 1.0 - p) | (r.l == r.m)) if p < 1 else surv
    assert np.array_equal(kept, r.valid & (r.l >= cut))            # the kept set is a threshold on the logit
    return kept, ratio, t_k


def rows(cols, g):
    """name -> fp32 row [cols]: N(0, std) for std in STDS, the `neg_inf` and `dominant` rows of tests/test_gpu_sample.py, and an all-equal
    row.  (The tie row depends on k: tie_row.)"""
    out = _sample_rows(cols, g)
    out["all_equal"] = torch.full((cols,), 0.75)
    return out


def tie_row(cols, k, g):
    """A N(0, 2) row whose k-th largest value stands three times, straddling the k boundary: sorted descending, positions k - 2, k - 1 and
    k (0-based) hold the same value — two copies inside the first k, one outside (for k = 1: positions 0, 1, 2), at shuffled columns."""
    assert cols >= 3 and 1 <= k <= cols - 1
    v = torch.sort(torch.randn(cols, generator=g) * 2, descending=True).values
    first = max(k - 2, 0)
    v[first:first + 3] = v[first + 1].clone()
    return v[torch.randperm(cols, generator=g)]
