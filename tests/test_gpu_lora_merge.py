"""mp_lora_merge_rows_bf16 / mp_lora_merge_rows_batched against their contract
    Wdst[rows[o], c] = bf16(float(Wsrc[rows[o], c]) + scaling * sum_j b[o, j] a[j, c])        (fp32 sum from zero)
at the smallest shapes where the kernel can go wrong: a column count below, at and off the 512-column strip, more rows than one wave
walks at once and fewer than four, the fused-matrix row maps (gate interleave, the v third), ranks on the register path (8, 16) and on the
generic one (24, 64), the strides of the training copies ([W | scaling B]: fin + 64) and of ops.padded_rows, in place, and the table form.

Exact test: a in {-4..4} 2^-8, b in {-4..4} 2^-6, scaling in {1, 2}, W = bf16(0.02 randn).  Every product and partial sum is a multiple of
2^-14 of magnitude at most 64 * 16 * 2^-14 = 2^-4: exact in fp32 in ANY order, and so is the scaling by 1 or 2.  The last step adds W (8
significant bits, |W| < 2^-3) with ONE fp32 rounding, in the kernel (an fma) as on the CPU, and that rounding is exact wherever
|W| >= 2^-19 (the sum then spans less than 24 bits).  So the result must equal the CPU's (W.float() + scaling * (b @ a)).to(bf16) bit for
bit; that a float64 product, and a chain started from W in reversed order, give those bits too is asserted on the CPU in the test itself.

Bounded test: random a ~ U(+-1/sqrt(fin)), b ~ 0.05 randn.  v = the float64 value, e = (r + 2) 2^-24 (|W| + scaling sum_j |b_oj a_jc|): one fp32
rounding per product, per add, for the scale and for the final add (an fma only removes roundings).  The output must lie between bf16(v - e)
and bf16(v + e); at most 1 % of the elements may have two admissible values there (a CPU fp32 reference has 0.06 - 0.16 %)."""
import pytest
import torch

from kernel_parity import assert_bits, bf, canary_intact, canary_view, gen
from medplib_amd import ops

pytestmark = pytest.mark.gpu


def _gate_rows(n):
    c = torch.arange(n)
    return (c // 32) * 64 + c % 32


# name -> (fout, fin, r, rows or None (identity), rows of the whole matrix, source row stride - fin, destination row stride - fin, scaling)
CASES = {
    "identity-64x64-r8": (64, 64, 8, None, 64, 64, 0, 2.0),
    "gate-interleave-320x256-r8": (320, 256, 8, _gate_rows(320), 640, 64, 320, 2.0),
    "v-third-256x320-r16": (256, 320, 16, torch.arange(256) + 512, 768, 64, 0, 1.0),
    "ragged-strip-48x520-r8": (48, 520, 8, None, 48, 64, 320, 2.0),
    "k4096-16-rows-r16": (16, 4096, 16, None, 16, 64, 0, 1.0),
    "k11008-16-rows-r8": (16, 11008, 8, None, 16, 64, 320, 2.0),
    "three-rows-r8": (3, 1024, 8, torch.tensor([5, 0, 2]), 7, 0, 0, 2.0),
    "r24": (40, 576, 24, None, 40, 64, 0, 1.0),
    # (at r = 64 the bound e is 66 roundings wide: a long K and scaling 1 keep the share of two-valued elements of the bounded test below its 1 %)
    "r64": (8, 8192, 64, torch.arange(8) * 2 + 1, 16, 64, 320, 1.0),
}


def _dyadic(fout, fin, r, seed):
    g = gen(seed)
    a = torch.randint(-4, 5, (r, fin), generator=g).float() * 2.0 ** -8
    b = torch.randint(-4, 5, (fout, r), generator=g).float() * 2.0 ** -6
    return a, b


def _random(fout, fin, r, seed):
    g = gen(seed)
    a = (torch.rand(r, fin, generator=g) * 2 - 1) / fin ** 0.5
    b = 0.05 * torch.randn(fout, r, generator=g)
    return a, b


def _weights(W, fin, seed):
    return (0.02 * torch.randn(W, fin, generator=gen(seed))).bfloat16()


def _launch(dev, w, a, b, rows, scaling, pad_src, pad_dst, in_place=False):
    """-> (destination on the CPU, whole destination buffer, source view on the device): the source as a [W, fin] view of row stride fin + pad_src,
    the destination as one of row stride fin + pad_dst inside a canary buffer, pre-filled with the source's rows (the kernel leaves the others)."""
    W, fin = w.shape
    whole_s, src = canary_view(W, fin, fin + pad_src, torch.bfloat16, dev)
    src.copy_(w.to(dev))
    if in_place:
        whole_d, dst = whole_s, src
    else:
        whole_d, dst = canary_view(W, fin, fin + pad_dst, torch.bfloat16, dev)
        dst.fill_(3.0)                                       # rows the adapter does not name must keep this
    ops.lora_merge_rows(src, dst, a.to(dev), b.to(dev), rows.to(dev), scaling)
    torch.cuda.synchronize()
    return dst.cpu(), whole_d, src


def _expected(w, a, b, rows, scaling, untouched):
    out = torch.full_like(w, untouched) if untouched is not None else w.clone()
    out[rows] = (w[rows].float() + scaling * (b @ a)).to(torch.bfloat16)
    return out


def _case(name):
    fout, fin, r, rows, W, pad_src, pad_dst, scaling = CASES[name]
    rows = torch.arange(fout) if rows is None else rows
    assert rows.numel() == fout and int(rows.max()) < W and int(rows.min()) >= 0 and rows.unique().numel() == fout
    return fout, fin, r, rows, W, pad_src, pad_dst, scaling


@pytest.mark.parametrize("name", list(CASES))
def test_exact_on_dyadic_adapters(dev, name):
    fout, fin, r, rows, W, pad_src, pad_dst, scaling = _case(name)
    a, b = _dyadic(fout, fin, r, 11)
    w = _weights(W, fin, 12)
    ref = _expected(w, a, b, rows, scaling, 3.0)
    # the claim the test rests on, checked where it is made: fp32, float64 and a chain started from W agree bit for bit on the CPU
    ref64 = (w[rows].double() + scaling * (b.double() @ a.double())).to(torch.bfloat16)
    chain = w[rows].float()
    for j in reversed(range(r)):
        chain = chain + scaling * b[:, j:j + 1] * a[j:j + 1]
    assert torch.equal(ref[rows], ref64) and torch.equal(ref[rows], chain.to(torch.bfloat16))
    changed = float((ref[rows] != w[rows]).float().mean())
    print(f"{name}: {changed:.3f} of the merged elements differ from W")
    assert changed > 0.9
    got, whole, src = _launch(dev, w, a, b, rows, scaling, pad_src, pad_dst)
    assert_bits(name, got, ref)
    canary_intact(name, whole, W, fin, fin + pad_dst)
    assert torch.equal(src.cpu(), w)                                # the source is read only


@pytest.mark.parametrize("name", list(CASES))
def test_bounded_on_random_adapters(dev, name):
    fout, fin, r, rows, W, pad_src, pad_dst, scaling = _case(name)
    a, b = _random(fout, fin, r, 21)
    w = _weights(W, fin, 22)
    got, whole, _ = _launch(dev, w, a, b, rows, scaling, pad_src, pad_dst)
    canary_intact(name, whole, W, fin, fin + pad_dst)
    w64 = w[rows].double()
    v = w64 + scaling * (b.double() @ a.double())
    e = (r + 2) * 2.0 ** -24 * (w64.abs() + scaling * (b.double().abs() @ a.double().abs()))
    lo, hi = bf((v - e).float()).double(), bf((v + e).float()).double()
    g = got[rows].double()
    two = float((lo != hi).double().mean())
    bad = int(((g < lo) | (g > hi)).sum())
    cpu32 = (w[rows].float() + scaling * (b @ a)).to(torch.bfloat16).double()
    print(f"{name}: {bad}/{g.numel()} outside [bf16(v - e), bf16(v + e)], {two:.5f} of the elements have two admissible values, "
          f"{int((g != cpu32).sum())} differ from the CPU's fp32 result")
    assert two <= 0.01, two
    assert bad == 0
    keep = torch.ones(W, dtype=torch.bool)
    keep[rows] = False
    assert bool((got[keep] == 3.0).all())                           # rows the adapter does not name


def test_capped_grid_walks_whole_batches_and_a_tail(dev):
    """The one size at which a wave of the single form walks more than eight rows: the grid stops growing at 2048 workgroups (8192 waves), so
    81920 rows of one 512-column strip are ten per wave: whole batches of rows in flight, then two rows of the tail loop."""
    fout, fin, r, scaling = 81920, 512, 8, 2.0
    a, b = _dyadic(fout, fin, r, 51)
    w = _weights(fout, fin, 52)
    rows = torch.arange(fout - 1, -1, -1)                            # (reversed: row o of the adapter is not row o of the matrix)
    ref = _expected(w, a, b, rows, scaling, None)
    got, whole, _ = _launch(dev, w, a, b, rows, scaling, 64, 0)
    assert_bits("capped grid", got, ref)
    canary_intact("capped grid", whole, fout, fin, fin)


@pytest.mark.parametrize("name", ["gate-interleave-320x256-r8", "ragged-strip-48x520-r8", "r24"])
def test_in_place_deterministic_and_restorable(dev, name):
    fout, fin, r, rows, W, pad_src, _, scaling = _case(name)
    a, b = _dyadic(fout, fin, r, 31)
    w = _weights(W, fin, 32)
    ref = _expected(w, a, b, rows, scaling, None)
    got, whole, _ = _launch(dev, w, a, b, rows, scaling, pad_src, pad_src, in_place=True)
    assert_bits(name + " in place", got, ref)
    canary_intact(name + " in place", whole, W, fin, fin + pad_src)
    # two launches on random adapters: the same bits; then the pristine copy put back: the original matrix
    a, b = _random(fout, fin, r, 33)
    x = torch.zeros(W, fin + 64, dtype=torch.bfloat16, device=dev)           # the [W | scaling B] copy of the training forward
    x[:, :fin].copy_(w.to(dev))
    plain = w.to(dev).clone()
    first = ops.lora_merge_rows(x[:, :fin], plain, a.to(dev), b.to(dev), rows.to(dev), scaling).clone()
    ops.lora_merge_rows(x[:, :fin], plain, a.to(dev), b.to(dev), rows.to(dev), scaling)
    assert torch.equal(first, plain) and not torch.equal(plain.cpu(), w)
    plain.copy_(x[:, :fin])
    assert torch.equal(plain.cpu(), w) and bool((x[:, fin:] == 0).all())


def test_three_experts_through_the_table(dev):
    """Three experts' gate adapters of one [E, 2 ff, d] weight in one launch, ranks and scalings mixed, beside the single form's results."""
    E, ff, d = 3, 96, 256
    rows = _gate_rows(ff)
    whole_s, src = canary_view(E * 2 * ff, d, d + 64, torch.bfloat16, dev)
    whole_d, dst = canary_view(E * 2 * ff, d, d, torch.bfloat16, dev)
    w = _weights(E * 2 * ff, d, 41)
    src.copy_(w.to(dev))
    dst.copy_(w.to(dev))
    items, ref = [], w.clone()
    for e, (r, scaling) in enumerate(((8, 2.0), (16, 1.0), (24, 2.0))):
        a, b = _dyadic(ff, d, r, 42 + e)
        lo = e * 2 * ff
        items.append((src[lo:lo + 2 * ff], dst[lo:lo + 2 * ff], a.to(dev), b.to(dev), rows.to(dev), scaling))
        ref[lo + rows] = (w[lo + rows].float() + scaling * (b @ a)).to(torch.bfloat16)
    table, n = ops.lora_merge_table(items, dev)
    assert n == 3 and table.numel() == 3 * 72
    ops.lora_merge_rows_batched(table, n)
    torch.cuda.synchronize()
    assert_bits("table form", dst.cpu(), ref)
    canary_intact("table form", whole_d, E * 2 * ff, d, d)
    single = w.to(dev).clone()
    for s, _, a, b, rw, scaling in items:
        lo = (s.data_ptr() - src.data_ptr()) // (2 * (d + 64))
        ops.lora_merge_rows(s, single[lo:lo + 2 * ff], a, b, rw, scaling)
    assert torch.equal(single, dst)
