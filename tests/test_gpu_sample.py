"""mp_sample_rows_f32 (temperature sampling of the next token by inverse CDF) against a float64 reference written here in numpy.

The band: with C the float64 CDF of softmax(l / T) normalised to 1, the picked column k must have w_k > 0 and C[k-1] - d <= u <= C[k] + d,
d = 1e-4.  Equality with the float64 pick is not the test: a u within fp32 rounding of a CDF step legitimately lands on either side (a purely
sequential fp32 cumulative sum over 32000 columns disagrees with float64 in 1.4 % of such cases and stays within 2.9e-5 of the band)."""
import numpy as np
import pytest
import torch

from medplib_amd import ops

pytestmark = pytest.mark.gpu

D = 1e-4
COLS = (2, 63, 64, 1000, 32000, 32011, 65536)
TEMPS = (0.2, 0.7, 1.0)
BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))


def _cdf64(row, T):
    """(CDF normalised to 1, weights) of softmax(row / T) in float64; -inf columns weigh 0."""
    l = row.astype(np.float64)
    w = np.exp((l - l.max()) / T)
    c = np.cumsum(w)
    return c / c[-1], w


def _rows(cols, g):
    """name -> fp32 row: N(0, std) for std in {0.5, 2, 4, 8}, a row with -inf entries (first and last columns among them), a row with one
    dominant entry."""
    out = {}
    for std in (0.5, 2.0, 4.0, 8.0):
        out[f"std{std}"] = torch.randn(cols, generator=g) * std
    r = torch.randn(cols, generator=g) * 2
    r[torch.rand(cols, generator=g) < 0.3] = -float("inf")
    r[0] = r[-1] = -float("inf")
    if cols == 2:
        r[0] = 0.5                                               # (keep one finite column)
    else:
        r[cols // 2] = 1.0
    out["neg_inf"] = r
    r = torch.randn(cols, generator=g)
    r[(cols * 2) // 3] += 30.0
    out["dominant"] = r
    return out


def _uniforms(cdf, n, g):
    """0, the largest float below 1, 1 itself (the keyed generator draws it), values next to steps of the CDF, and random ones."""
    near = cdf[np.linspace(0, len(cdf) - 1, 12).astype(np.int64)].astype(np.float32)
    u = np.concatenate([[0.0, BELOW_ONE, 1.0, 0.5], near, np.nextafter(near, np.float32(0)), np.nextafter(near, np.float32(2)),
                        torch.rand(n, generator=g).numpy()]).astype(np.float32)
    return np.clip(u, 0.0, 1.0)


def _check_band(tok, u, cdf, w, case):
    tok = np.asarray(tok)
    assert tok.min() >= 0 and tok.max() < len(cdf), (case, tok.min(), tok.max())
    assert (w[tok] > 0).all(), (case, "a column with zero weight was picked")
    lo = np.where(tok > 0, cdf[np.maximum(tok - 1, 0)], 0.0)
    hi = cdf[tok]
    worst = max(float((lo - u).max()), float((u - hi).max()))
    assert worst <= D, (case, worst)
    return worst


def test_pick_is_inside_the_float64_band(dev):
    g = torch.Generator().manual_seed(11)
    worst, n_cases, exact = 0.0, 0, 0
    for cols in COLS:
        for name, row in _rows(cols, g).items():
            for T in TEMPS:
                cdf, w = _cdf64(row.numpy(), T)
                u = _uniforms(cdf, 40, g)
                logits = row.to(dev).view(1, cols).expand(len(u), cols)          # one row against every u (row stride 0)
                tok = ops.sample_rows(logits, torch.from_numpy(u).to(dev), T).cpu().numpy()
                worst = max(worst, _check_band(tok, u.astype(np.float64), cdf, w, (cols, name, T)))
                ref = np.minimum(np.searchsorted(cdf, u.astype(np.float64), side="right"), np.flatnonzero(w > 0)[-1])
                exact += int((ref == tok).sum()); n_cases += len(u)
    print(f"{n_cases} picks: worst distance outside the float64 CDF interval {worst:.3e} (band {D}); {exact} equal the float64 pick")
    assert n_cases == len(COLS) * 6 * len(TEMPS) * 80


def test_edges_of_the_cdf(dev):
    """u = 0 picks the first column with w > 0, u >= 1 the last one; never a -inf column, never a column past `cols`."""
    for cols in (2, 63, 32011, 65536):
        row = torch.zeros(cols)
        row[0] = row[-1] = -float("inf") if cols > 2 else 0.0
        u = torch.tensor([0.0, BELOW_ONE, 1.0, 2.0], device=dev)
        tok = ops.sample_rows(row.to(dev).view(1, cols).expand(4, cols), u, 1.0).cpu().tolist()
        first, last = (1, cols - 2) if cols > 2 else (0, 1)
        assert tok[0] == first and tok[2] == last and tok[3] == last and tok[1] in (last, last - 1), (cols, tok)


def test_rows_without_a_finite_entry_pick_column_zero(dev):
    """An all -inf row and an all-NaN row have no column with w > 0: the pick is 0 for every u — never one of the columns the kernel pads the
    row with up to 32768 / 65536.  NaN columns beside finite ones are never picked and the pick stays inside the row."""
    u = torch.tensor([0.0, 0.5, 0.98, BELOW_ONE, 1.0], device=dev)
    for cols in (2, 63, 32000, 32011, 40000, 65536):
        for fill in (-float("inf"), float("nan")):
            row = torch.full((1, cols), fill, device=dev)
            for T in (0.2, 1.0):
                assert ops.sample_rows(row.expand(5, cols), u, T).cpu().tolist() == [0] * 5, (cols, fill, T)
        if cols >= 63:
            row = torch.zeros(cols)
            row[5::7] = float("nan")
            row[-1] = float("nan")
            tok = ops.sample_rows(row.to(dev).view(1, cols).expand(5, cols), u, 1.0).cpu()
            assert int(tok.min()) >= 0 and int(tok.max()) < cols and not torch.isnan(row[tok]).any(), (cols, tok)
        # a batch whose rows differ: the degenerate rows do not disturb their neighbours
        batch = torch.zeros(3, cols)
        batch[0] = -float("inf"); batch[2] = float("nan")
        tok = ops.sample_rows(batch.to(dev), u[:3].contiguous(), 1.0).cpu().tolist()
        assert tok[0] == 0 and tok[2] == 0 and 0 <= tok[1] < cols, (cols, tok)


def test_same_inputs_same_columns_and_batch_equals_single_rows(dev):
    g = torch.Generator().manual_seed(12)
    for cols in (63, 1000, 32011):                       # 63 and 32011: rows of a batch start off 16 bytes
        R = 24
        logits = (torch.randn(R, cols, generator=g) * 3).to(dev)
        u = torch.rand(R, generator=g).to(dev)
        for T in (0.2, 1.0):
            a = ops.sample_rows(logits, u, T)
            b = ops.sample_rows(logits, u, T)
            single = torch.cat([ops.sample_rows(logits[r:r + 1].clone(), u[r:r + 1].clone(), T) for r in range(R)])
            assert torch.equal(a, b) and torch.equal(a, single), (cols, T)
            cdfs = [_cdf64(logits[r].cpu().numpy(), T) for r in range(R)]
            for r in range(R):
                _check_band(a[r:r + 1].cpu().numpy(), u[r:r + 1].cpu().numpy().astype(np.float64), *cdfs[r], (cols, T, r))


def test_distribution_of_200000_keyed_draws(dev):
    """One 64-column row, 200 000 uniforms of the keyed generator (fixed seed): Pearson's chi-square of the picked columns against the float64
    softmax stays below the 1 - 1e-6 quantile for 63 degrees of freedom (131.37)."""
    from scipy.stats import chi2
    n = 200000
    row = torch.randn(64, generator=torch.Generator().manual_seed(13))
    cdf, w = _cdf64(row.numpy(), 1.0)
    p = w / w.sum()
    u = ops.gate_noise(n, 1234, 0, False, dev)
    assert float(u.min()) > 0.0 and float(u.max()) <= 1.0
    tok = ops.sample_rows(row.to(dev).view(1, 64).expand(n, 64), u, 1.0).cpu().numpy()
    counts = np.bincount(tok, minlength=64).astype(np.float64)
    stat = float(((counts - n * p) ** 2 / (n * p)).sum())
    bound = float(chi2.ppf(1 - 1e-6, 63))
    print(f"chi-square {stat:.2f} (bound {bound:.2f}); smallest expected count {n * p.min():.1f}")
    assert abs(bound - 131.37) < 0.01 and stat < bound


def test_cold_limit_is_argmax(dev):
    """T -> 1e-4: on rows whose top-two logit gap is above 0.01 every u picks the argmax."""
    g = torch.Generator().manual_seed(14)
    checked = 0
    for cols in (64, 1000, 32000):
        logits = (torch.randn(32, cols, generator=g) * 2).to(dev)
        top2 = logits.cpu().topk(2, dim=1).values
        keep = (top2[:, 0] - top2[:, 1]) > 0.01
        for uval in (0.0, 0.37, BELOW_ONE, 1.0):
            tok = ops.sample_rows(logits, torch.full((32,), uval, device=dev), 1e-4)
            assert torch.equal(tok.cpu()[keep], ops.argmax_rows(logits).cpu()[keep]), (cols, uval)
        checked += int(keep.sum())
    assert checked > 48
