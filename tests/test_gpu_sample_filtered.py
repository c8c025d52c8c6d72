"""mp_sample_filtered_rows_f32 (top-k, then top-p truncation in front of the inverse-CDF pick) against the float64 rule of
tests/sample_filter_cases.py, which tests/test_sample_filtered_abi.py holds to HF's warper chain.

Top-k compares logits and is checked exactly.  Top-p and the pick sum fp32 weights, so they are checked inside the band of
tests/test_gpu_sample.py, d = 1e-4, placed on the boundary: the reported cut must satisfy A64(cut) / Z64 > 1 - p - d, and the next smaller
survivor logit t' must satisfy A64(t') / Z64 <= 1 - p + d.  (The kernel's sums stay within a few 1e-7 of float64 relative to Z: 52 fp32
additions deep, and __expf's ~1e-6 relative error on every weight.)  The pick is held to the float64 CDF renormalised over the kernel's own
kept set {l >= cut}, with the same d."""
import numpy as np
import pytest
import torch

from medplib_amd import ops
from sample_filter_cases import Row64, rows, tie_row
from test_gpu_sample import BELOW_ONE, COLS, D, TEMPS, _check_band, _uniforms

pytestmark = pytest.mark.gpu

PS = (0.0, 1e-6, 0.1, 0.5, 0.9, 0.999, 1.0)


def _ks(cols):
    return sorted({0, 1, 2, 50, cols - 1, cols, cols + 5})


def _launch(dev, row_dev, u, T, k, p):
    """One row against every u (row stride 0) -> (tokens, kept, cut) on the host; kept and cut are the same for every u."""
    n = len(u)
    tok, kept, cut = ops.sample_rows_filtered(row_dev.view(1, -1).expand(n, row_dev.numel()), torch.from_numpy(u).to(dev), T, k, p, want_cut=True)
    tok, kept, cut = tok.cpu().numpy(), kept.cpu().numpy(), cut.cpu().numpy()
    assert (kept == kept[0]).all() and (cut == cut[0]).all()
    return tok, int(kept[0]), float(cut[0])


def _check_case(dev, r64, row_dev, T, k, p, g, case):
    """Every check of one (row, T, k, p): the cut (exact for top-k alone, the band for top-p), kept, and the pick at _uniforms' values."""
    l, cols = r64.l, r64.cols
    cut64, t_k = r64.cut(k, p)
    mask64 = r64.valid & (l >= cut64)
    w64 = np.where(mask64, r64.w, 0.0)
    u = _uniforms(np.cumsum(w64) / w64.sum(), 12, g)
    tok, kept, cut = _launch(dev, row_dev, u, T, k, p)
    mask = r64.valid & (l >= cut)
    assert kept == int(mask.sum()) and cut in r64.ls, (case, kept, cut)
    worst = 0.0
    if p >= 1:                                                   # top-k alone (or nothing): exact
        assert cut == t_k and np.array_equal(mask, r64.valid & (l >= t_k)), (case, cut, t_k)
    else:
        assert cut >= t_k, (case, cut, t_k)
        at, under = r64.ratio(cut, t_k), r64.below(cut, t_k)
        assert at > 1.0 - p - D, (case, cut, at)
        worst = max(worst, (1.0 - p) - at)
        if under is not None:
            below = r64.ratio(under, t_k)
            assert below <= 1.0 - p + D, (case, cut, under, below)
            worst = max(worst, below - (1.0 - p))
    if not 0 < k < cols and p >= 1:                              # filters off: the plain pick, bit for bit
        plain = ops.sample_rows(row_dev.view(1, -1).expand(len(u), cols), torch.from_numpy(u).to(dev), T).cpu().numpy()
        assert np.array_equal(tok, plain), case
    wk = np.where(mask, r64.w, 0.0)
    _check_band(tok, u.astype(np.float64), np.cumsum(wk) / wk.sum(), wk, case)       # (w > 0 at the token: it is a kept column)
    return worst


@pytest.mark.parametrize("cols", COLS)
def test_cut_kept_and_pick_against_the_float64_rule(dev, cols):
    g = torch.Generator().manual_seed(31 + cols)
    worst, n = 0.0, 0
    cases = dict(rows(cols, g))
    ks = _ks(cols)
    for k in ks:
        if cols >= 3 and 1 <= k <= cols - 1:
            cases[f"tie{k}"] = tie_row(cols, k, g)
    for name, row in cases.items():
        row_dev = row.to(dev)
        for T in TEMPS:
            r64 = Row64(row.numpy(), T)
            for k in ([int(name[3:])] if name.startswith("tie") else ks):
                for p in PS:
                    worst = max(worst, _check_case(dev, r64, row_dev, T, k, p, g, (cols, name, T, k, p)))
                    n += 1
    print(f"cols {cols}: {n} cases; worst excursion of A/Z past 1 - p: {worst:.3e} (band {D})")


def test_ties_at_the_k_boundary_all_survive(dev):
    g = torch.Generator().manual_seed(32)
    u = np.asarray([0.0, 0.5, 1.0], dtype=np.float32)
    for cols in (63, 1000, 32011, 65536):
        for k in (1, 2, 50, cols - 1):
            row = tie_row(cols, k, g)
            t_k = float(torch.sort(row, descending=True).values[k - 1])
            assert int((row == t_k).sum()) == 3
            _, kept, cut = _launch(dev, row.to(dev), u, 0.7, k, 1.0)
            assert cut == t_k and kept == int((row >= t_k).sum()) == (k + 1 if k >= 2 else 3), (cols, k, kept, cut)


def test_filters_off_is_the_plain_pick_bit_for_bit(dev):
    """(k, p) in {(0, 1), (cols, 1), (cols + 5, 1)}, without the diagnostic outputs (one launch: the plain kernel's) and with them."""
    g = torch.Generator().manual_seed(33)
    for cols in COLS:
        for name, row in rows(cols, g).items():
            row_dev = row.to(dev).view(1, cols)
            for T in TEMPS:
                r64 = Row64(row.numpy(), T)
                u = torch.from_numpy(_uniforms(np.cumsum(r64.w) / r64.w.sum(), 20, g)).to(dev)
                logits = row_dev.expand(len(u), cols)
                plain = ops.sample_rows(logits, u, T)
                for k in (0, cols, cols + 5):
                    assert torch.equal(ops.sample_rows_filtered(logits, u, T, k, 1.0), plain), (cols, name, T, k)
                    tok, kept, cut = ops.sample_rows_filtered(logits, u, T, k, 1.0, want_cut=True)
                    assert torch.equal(tok, plain) and int(kept[0]) == cols and float(cut[0]) == float(row.min()), (cols, name, T, k)


def test_top_k_1_and_top_p_0_are_argmax(dev):
    """top_k = 1, and separately top_p in {0, 1e-6}, pick the argmax for every u on rows whose top-two gap is above 0.01 (at p = 1e-6 the
    runner-up's A / Z is at most 1 - 1 / Z <= 1 - 1.5e-5 for Z <= 65536); on the all-equal row every column is kept."""
    g = torch.Generator().manual_seed(34)
    checked = 0
    for cols in (64, 1000, 32000):
        logits = (torch.randn(32, cols, generator=g) * 2).to(dev)
        top2 = logits.cpu().topk(2, dim=1).values
        keep = (top2[:, 0] - top2[:, 1]) > 0.01
        ref = ops.argmax_rows(logits).cpu()[keep]
        for uval in (0.0, 0.37, BELOW_ONE, 1.0):
            u = torch.full((32,), uval, device=dev)
            for T in (0.2, 1.0):
                for k, p in ((1, 1.0), (0, 0.0), (0, 1e-6), (50, 0.0)):
                    tok, kept, cut = ops.sample_rows_filtered(logits, u, T, k, p, want_cut=True)
                    assert torch.equal(tok.cpu()[keep], ref), (cols, uval, T, k, p)
                    assert (kept.cpu()[keep] == 1).all() and torch.equal(cut.cpu()[keep], top2[:, 0][keep]), (cols, uval, T, k, p)
        checked += int(keep.sum())
    assert checked > 48
    for cols in (2, 63, 32011, 65536):
        row = torch.full((1, cols), -1.25, device=dev)
        for k, p in ((1, 1.0), (0, 0.0), (0, 1e-6), (2, 0.5)):
            tok, kept, cut = ops.sample_rows_filtered(row.expand(3, cols), torch.tensor([0.0, 0.5, 1.0], device=dev), 0.7, k, p, want_cut=True)
            assert kept.cpu().tolist() == [cols] * 3 and cut.cpu().tolist() == [-1.25] * 3, (cols, k, p)
            assert tok.cpu().tolist()[0] == 0 and tok.cpu().tolist()[2] == cols - 1, (cols, k, p, tok)


def test_same_inputs_same_tokens_and_batch_equals_single_rows(dev):
    g = torch.Generator().manual_seed(35)
    for cols in (63, 32011):                             # rows of a batch start off 16 bytes
        R = 24
        logits = (torch.randn(R, cols, generator=g) * 3).to(dev)
        u = torch.rand(R, generator=g).to(dev)
        for T, k, p in ((0.2, 50, 0.9), (1.0, 0, 0.9), (0.7, 5, 1.0)):
            a = ops.sample_rows_filtered(logits, u, T, k, p, want_cut=True)
            b = ops.sample_rows_filtered(logits, u, T, k, p, want_cut=True)
            single = [ops.sample_rows_filtered(logits[r:r + 1].clone(), u[r:r + 1].clone(), T, k, p, want_cut=True) for r in range(R)]
            for i in range(3):
                assert torch.equal(a[i], b[i]) and torch.equal(a[i], torch.cat([s[i] for s in single])), (cols, T, k, p, i)
            # ld = 0: one row against every u equals that row's own launches
            bro = ops.sample_rows_filtered(logits[3:4].expand(R, cols), u, T, k, p, want_cut=True)
            own = [ops.sample_rows_filtered(logits[3:4].clone(), u[r:r + 1].clone(), T, k, p, want_cut=True) for r in range(R)]
            for i in range(3):
                assert torch.equal(bro[i], torch.cat([s[i] for s in own])), (cols, T, k, p, i)


def test_distribution_of_200000_keyed_draws_over_the_kept_set(dev):
    """One 64-column row, k = 8, p = 0.8, 200 000 uniforms of the keyed generator in one ld = 0 launch: no token outside the kernel's own kept
    set, and Pearson's chi-square against the float64 distribution renormalised over it below the 1 - 1e-6 quantile for kept - 1 degrees."""
    from scipy.stats import chi2
    n = 200000
    row = torch.randn(64, generator=torch.Generator().manual_seed(13))
    r64 = Row64(row.numpy(), 1.0)
    u = ops.gate_noise(n, 1234, 0, False, dev)
    tok, kept, cut = ops.sample_rows_filtered(row.to(dev).view(1, 64).expand(n, 64), u, 1.0, 8, 0.8, want_cut=True)
    tok, kept, cut = tok.cpu().numpy(), int(kept[0]), float(cut[0])
    mask = r64.l >= cut
    assert 2 <= kept == int(mask.sum()) <= 8 and mask[tok].all()
    prob = r64.w[mask] / r64.w[mask].sum()
    counts = np.bincount(tok, minlength=64).astype(np.float64)[mask]
    stat = float(((counts - n * prob) ** 2 / (n * prob)).sum())
    bound = float(chi2.ppf(1 - 1e-6, kept - 1))
    print(f"kept {kept}: chi-square {stat:.2f} (bound {bound:.2f}); smallest expected count {n * prob.min():.1f}")
    assert stat < bound


def test_degenerate_rows(dev):
    """All -inf and all NaN: token 0, kept 0, cut +inf, beside ordinary rows too; NaN columns beside finite ones are never kept; rows = 0
    is fine."""
    u = torch.tensor([0.0, 0.5, 0.98, BELOW_ONE, 1.0], device=dev)
    for cols in (2, 63, 32000, 32011, 40000, 65536):
        for fill in (-float("inf"), float("nan")):
            row = torch.full((1, cols), fill, device=dev)
            for k, p in ((50, 0.9), (0, 0.5), (1, 1.0), (0, 1.0)):
                tok, kept, cut = ops.sample_rows_filtered(row.expand(5, cols), u, 0.7, k, p, want_cut=True)
                assert tok.cpu().tolist() == [0] * 5 and kept.cpu().tolist() == [0] * 5, (cols, fill, k, p)
                assert cut.cpu().tolist() == [float("inf")] * 5, (cols, fill, k, p)
        if cols >= 63:
            row = torch.arange(cols, dtype=torch.float32) * 1e-3
            row[5::7] = float("nan")
            row[-1] = float("nan")
            n_nan = int(torch.isnan(row).sum())
            tok, kept, cut = ops.sample_rows_filtered(row.to(dev).view(1, cols).expand(5, cols), u, 1.0, 0, 0.9999, want_cut=True)
            assert not torch.isnan(row[tok.cpu()]).any() and (row[tok.cpu()] >= cut.cpu()).all(), (cols, tok)
            tok, kept, cut = ops.sample_rows_filtered(row.to(dev).view(1, cols).expand(5, cols), u, 1.0, cols - 1, 1.0, want_cut=True)
            assert kept.cpu().tolist() == [cols - n_nan] * 5 and not torch.isnan(row[tok.cpu()]).any(), (cols, kept)    # k past the non-NaN count
        batch = torch.zeros(3, cols)
        batch[0] = -float("inf"); batch[2] = float("nan")
        tok, kept, cut = ops.sample_rows_filtered(batch.to(dev), u[:3].contiguous(), 1.0, 1, 0.9, want_cut=True)
        assert tok.cpu().tolist()[0] == 0 and tok.cpu().tolist()[2] == 0 and kept.cpu().tolist() == [0, cols, 0], (cols, tok, kept)
    empty = ops.sample_rows_filtered(torch.empty(0, 100, device=dev), torch.empty(0, device=dev), 1.0, 5, 0.5)
    assert empty.shape == (0,)
