"""mp_pick_rows_f32: one pick launch whose rows each bring their own temperature, top_k and top_p, and mp_gate_noise_rows_dev_f32, the rows'
draws under their own seeds.  The contract is bits, so every comparison is torch.equal and the oracle is the existing single-row op on the
row alone: ops.argmax_rows (inv_temperature 0), ops.sample_rows (filters off) or ops.sample_rows_filtered."""
import itertools

import pytest
import torch

from medplib_amd import ops

pytestmark = pytest.mark.gpu

COLS = (1, 3, 4, 5, 4096, 4099, 32768, 32769, 65536)      # one column, a straddling piece, one piece per thread, K = 8 | K = 16 on both sides
ROWS = (1, 3, 8, 9)                                        # (9: there is no 8-row limit in the kernel)
NAN, INF = float("nan"), float("inf")
# (temperature or None = greedy, top_k or a function of cols, top_p)
KINDS = ((None, 0, 1.0), (0.7, 0, 1.0), (1.3, 0, 1.0), (0.7, 5, 1.0), (0.7, 0, 0.9), (1.3, 5, 0.9), (0.7, lambda cols: cols + 3, 1.0),
         (0.7, 0, 0.0), (1.3, 1, 1.0))


def _kind(i, cols):
    T, k, p = KINDS[i % len(KINDS)]
    return T, (k(cols) if callable(k) else k), p


def _params(kinds, dev):
    """The device arrays of a launch whose row r has kinds[r] = (T, k, p)."""
    inv_t = torch.tensor([0.0 if T is None else 1.0 / T for T, _, _ in kinds], dtype=torch.float32).to(dev)
    return inv_t, torch.tensor([k for _, k, _ in kinds], dtype=torch.int32).to(dev), torch.tensor([p for _, _, p in kinds], dtype=torch.float32).to(dev)


def _alone(row, u, kind):
    """The existing op that serves `kind` on one row [1, cols] alone -> its token (an int)."""
    T, k, p = kind
    cols = row.shape[1]
    if T is None:
        if not bool((row == row).any()):                   # no non-NaN column: the stated rule (mp_argmax_rows_f32 leaves it undefined)
            return 0
        return int(ops.argmax_rows(row)[0])
    if not 0 < k < cols and p >= 1.0:
        return int(ops.sample_rows(row, u, T)[0])
    return int(ops.sample_rows_filtered(row, u, T, k, p)[0])


def _expected(logits, u, kinds):
    return torch.tensor([_alone(logits[r:r + 1], u[r:r + 1].clone(), kinds[r]) for r in range(logits.shape[0])], dtype=torch.int64)


def _buffer(rows, cols, ld, g, dev):
    """fp32 [rows, cols] with row stride ld on the device (ld = cols + 1: rows start off 16 bytes)."""
    buf = (torch.randn(rows, ld, generator=g) * 3).to(dev)
    return buf[:, :cols]


def _draws(rows, g, dev):
    u = torch.rand(rows, generator=g)
    u[0] = 2.0 ** -25
    if rows > 1:
        u[-1] = 1.0
    return u.to(dev)


@pytest.mark.parametrize("cols", COLS)
def test_every_row_has_the_token_of_the_op_that_serves_it(dev, cols):
    g = torch.Generator().manual_seed(71 + cols)
    offset = itertools.count()
    seen = set()
    for rows in ROWS:
        for ld in (cols, cols + 1):
            logits = _buffer(rows, cols, ld, g, dev)
            assert logits.stride(0) == ld
            u = _draws(rows, g, dev)
            first = next(offset) * 2
            kinds = [_kind(first + r, cols) for r in range(rows)]
            seen.update((first + r) % len(KINDS) for r in range(rows))
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            got = ops.pick_rows(logits, u, *_params(kinds, dev), err)
            assert got.dtype == torch.int64 and torch.equal(got.cpu(), _expected(logits, u, kinds)), (cols, rows, ld, kinds)
            assert int(err[0]) == 0
    assert seen == set(range(len(KINDS)))                  # every kind ran beside others


def _special_rows(cols):
    out = {"all -inf": torch.full((cols,), -INF), "all nan": torch.full((cols,), NAN)}
    g = torch.Generator().manual_seed(5 + cols)
    r = torch.randn(cols, generator=g) * 3
    r[0] = NAN
    r[cols // 2] = NAN
    out["nan beside finite"] = r
    r = torch.randn(cols, generator=g).clamp(max=2.0)
    r[cols // 3] = r[cols - 1] = 4.5
    out["two equal maxima"] = r
    r = torch.randn(cols, generator=g)
    r[cols - 2] = INF
    out["+inf maximum"] = r
    return out


@pytest.mark.parametrize("cols", (3, 4099, 32769))
def test_special_rows_under_every_kind(dev, cols):
    g = torch.Generator().manual_seed(9)
    n = len(KINDS)
    kinds = [_kind(i, cols) for i in range(n)]
    for name, row in _special_rows(cols).items():
        for ld in (cols, cols + 1):
            buf = torch.zeros(n, ld)
            buf[:, :cols] = row
            logits = buf.to(dev)[:, :cols]
            u = _draws(n, g, dev)
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            got = ops.pick_rows(logits, u, *_params(kinds, dev), err).cpu()
            want = _expected(logits, u, kinds)
            assert torch.equal(got, want), (cols, name, ld, got, want)
            assert int(err[0]) == 0
            if name in ("all -inf", "all nan"):
                assert got.tolist() == [0] * n, (cols, name)
            if name == "two equal maxima":
                assert int(got[0]) == cols // 3                 # greedy: the first of the two
            if name == "+inf maximum":
                assert int(got[0]) == cols - 2


def test_rows_are_independent_and_launches_repeat(dev):
    g = torch.Generator().manual_seed(12)
    for cols in (4099, 32769):
        rows = 9
        logits = _buffer(rows, cols, cols + 1, g, dev)
        u = _draws(rows, g, dev)
        kinds = [_kind(r, cols) for r in range(rows)]
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        a = ops.pick_rows(logits, u, *_params(kinds, dev), err)
        assert torch.equal(a, ops.pick_rows(logits, u, *_params(kinds, dev), err))
        perm = torch.randperm(rows, generator=g)
        moved = logits.index_select(0, perm.to(dev))           # (contiguous: another stride and alignment as well)
        b = ops.pick_rows(moved, u[perm.to(dev)].contiguous(), *_params([kinds[int(i)] for i in perm], dev), err)
        assert torch.equal(b, a[perm.to(dev)]) and int(err[0]) == 0


@pytest.mark.parametrize("bad", ("inv_t -1", "inv_t nan", "inv_t inf", "top_p 1.5", "top_p nan", "top_k -1"))
def test_a_refused_row_sets_the_error_bit_and_leaves_the_others(dev, bad):
    g = torch.Generator().manual_seed(13)
    cols, rows, at = 4099, 4, 2
    logits = _buffer(rows, cols, cols, g, dev)
    u = _draws(rows, g, dev)
    kinds = [_kind(r + 1, cols) for r in range(rows)]
    inv_t, top_k, top_p = _params(kinds, dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    clean = ops.pick_rows(logits, u, inv_t, top_k, top_p, err)
    assert int(err[0]) == 0 and torch.equal(clean.cpu(), _expected(logits, u, kinds))
    which, value = bad.split()
    {"inv_t": inv_t, "top_p": top_p, "top_k": top_k}[which][at] = float(value) if which != "top_k" else int(value)
    err[0] = 1                                                 # (a bit another kernel set stays)
    got = ops.pick_rows(logits, u, inv_t, top_k, top_p, err)
    assert int(err[0]) == (1 | ops.POS_ERR_PICK) and int(got[at]) == 0
    keep = [r for r in range(rows) if r != at]
    assert torch.equal(got[keep], clean[keep])


def test_draws_are_the_keyed_generators(dev):
    seeds = [0, 1, 5, 2 ** 31 - 2, 2 ** 40 + 7]
    seeds_dev = torch.tensor(seeds, dtype=torch.int64).to(dev)
    for step in (0, 1, 17, 4095):
        got = ops.sample_uniform_rows(seeds_dev, step)
        assert got.dtype == torch.float32 and got.shape == (len(seeds),)
        want = torch.cat([ops.gate_noise(1, s, step, False, dev) for s in seeds])
        assert torch.equal(got, want), step
        assert torch.equal(want, torch.cat([ops.sample_uniform(s, step, dev) for s in seeds]))
    counter = torch.tensor([3], dtype=torch.int32, device=dev)
    for step in (3, 4, 5):
        got = ops.sample_uniform_rows(seeds_dev, counter)
        assert torch.equal(got, torch.cat([ops.gate_noise(1, s, step, False, dev) for s in seeds])), step
        ops.advance_ints(counter, 1)
    assert ops.sample_uniform_rows(seeds_dev[:0].contiguous(), 0).shape == (0,)


def test_a_captured_launch_serves_what_the_arrays_hold_at_replay(dev):
    g = torch.Generator().manual_seed(14)
    cols, rows = 4099, 5
    logits = _buffer(rows, cols, cols + 1, g, dev)
    kinds = [_kind(r, cols) for r in range(rows)]
    inv_t, top_k, top_p = _params(kinds, dev)
    seeds = torch.arange(100, 100 + rows, dtype=torch.int64).to(dev)
    step = torch.tensor([0], dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty(rows, dtype=torch.int64, device=dev)
    u_out = torch.empty(rows, dtype=torch.float32, device=dev)

    def launch():
        u = ops.sample_uniform_rows(seeds, step)
        u_out.copy_(u)
        out.copy_(ops.pick_rows(logits, u, inv_t, top_k, top_p, err))

    launch()                                                   # (eager once: nothing is initialised inside the capture)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            launch()
    torch.cuda.current_stream().wait_stream(side)

    def eager():
        u = ops.sample_uniform_rows(seeds, step)
        return u, ops.pick_rows(logits, u, inv_t, top_k, top_p, err)

    graph.replay()
    u0, t0 = eager()
    assert torch.equal(out, t0) and torch.equal(u_out, u0)
    # other requests in the same rows, a later token: nothing of the first ones is frozen into the graph
    new = [_kind(r + 4, cols) for r in range(rows)]
    a, b, c = _params(new, dev)
    inv_t.copy_(a); top_k.copy_(b); top_p.copy_(c)
    seeds.add_(1000)
    ops.advance_ints(step, 1); ops.advance_ints(step, 1)
    logits.copy_(_buffer(rows, cols, cols + 1, g, dev))
    graph.replay()
    u1, t1 = eager()
    assert int(step[0]) == 2 and torch.equal(u_out, u1) and not torch.equal(u1, u0)
    assert torch.equal(out, t1) and torch.equal(t1.cpu(), _expected(logits, u1, new))
    assert int(err[0]) == 0
