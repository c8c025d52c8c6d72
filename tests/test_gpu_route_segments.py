"""ops.moe_route_top1_segments / moe_route_top2_segments: the right-padded prompts of one batched prefill, each routed as a pass of its own.
The contract is exact: per segment, every output is the unsegmented op's on that segment's rows alone (integers ==, floats torch.equal), a
kept slot shifted behind the rows that earlier segments keep for the same expert.  Pad rows of the inputs hold NaN throughout: they are
never read."""
import ctypes
import math

import pytest
import torch

from medplib_amd import _lib, ops

pytestmark = pytest.mark.gpu

# (segment lengths, stride): one segment of one token; a wave-sized, a single-token and a full-wave segment (the one-wave form at its edge);
# the 1024-thread register form from 65 tokens, at a chunk of one, at 1023 / 1025 (the chunk of two) and beside a short one; the
# non-register form past 16 * 1024 tokens; eight segments of mixed length under a stride longer than any of them
SHAPES = {
    "one": ((1,), 1),
    "wave": ((9, 1, 64), 64),
    "block": ((65, 1023, 1025, 7), 1025),
    "long": ((16385, 3), 16385),
    "eight": ((5, 64, 65, 200, 1, 130, 77, 300), 304),
}
CASES = [(s, E) for s in ("one", "wave", "block", "eight") for E in (2, 3, 8)] + [("long", 2)]
CAPS = ("cf2.0", "cf0.5", "one", "full")


def _capacities(lens, E, top_k, mode):
    """LlamaStack.capacity's formula (min_capacity = 0) at factor 2.0 (top-1: nothing can drop) and 0.5 (drops), and two hand-set ones."""
    if mode.startswith("cf"):
        return [int(math.ceil(n / E * float(mode[2:]) * top_k)) for n in lens]
    return [1 if mode == "one" else n + 3 for n in lens]


def _inputs(dev, lens, stride, E):
    """Seeded softmax gates of normal logits; segment 1 (or the only one) names expert 0 with every token; the last segment of several has
    exactly equal gates (the first index wins); NaN in every pad row."""
    g = torch.Generator().manual_seed(17 * len(lens) + E + stride)
    logits = torch.randn((len(lens) * stride, E), generator=g)
    crafted = min(1, len(lens) - 1)
    logits[crafted * stride:(crafted + 1) * stride, 0] += 12.0
    if len(lens) > 1:
        logits[(len(lens) - 1) * stride:] = 0.0
    gates = torch.softmax(logits, dim=1)
    for b, n in enumerate(lens):
        logits[b * stride + n:(b + 1) * stride] = float("nan")
        gates[b * stride + n:(b + 1) * stride] = float("nan")
    return gates.to(dev).contiguous(), logits.to(dev).contiguous()


def _check(dev, top_k, lens, stride, E, caps):
    gates, logits = _inputs(dev, lens, stride, E)
    T = len(lens) * stride
    if top_k == 1:
        expert, slot, weight, kept, counts, l_aux, slot_token = ops.moe_route_top1_segments(gates, lens, stride, caps, want_slot_token=True)
        assert slot_token.shape == (E, sum(caps))
    else:
        expert, slot, weight, kept, counts, l_aux = ops.moe_route_top2_segments(gates, logits, lens, stride, caps)
    assert expert.shape == slot.shape == weight.shape == (top_k * T,) and l_aux.shape == (len(lens),)
    assert bool(torch.isfinite(l_aux).all())
    base = torch.zeros(E, dtype=torch.int64, device=dev)
    counts_sum = torch.zeros(E, dtype=torch.int64, device=dev)
    pad = torch.ones(T, dtype=torch.bool, device=dev)
    some_dropped = False
    for b, (n, cap) in enumerate(zip(lens, caps)):
        rows = slice(b * stride, b * stride + n)
        pad[rows] = False
        if top_k == 1:
            r_expert, r_slot, r_weight, r_kept, r_counts, r_aux = ops.moe_route_top1(gates[rows].contiguous(), cap)
        else:
            r_expert, r_slot, r_weight, r_kept, r_counts, r_aux = ops.moe_route_top2(gates[rows].contiguous(), logits[rows].contiguous(), cap)
        for c in range(top_k):
            mine = slice(c * T + b * stride, c * T + b * stride + n)
            ref = slice(c * n, (c + 1) * n)
            assert torch.equal(expert[mine], r_expert[ref]), (b, c)
            assert torch.equal(weight[mine], r_weight[ref]), (b, c)
            dropped = r_slot[ref] < 0
            assert torch.equal(slot[mine] < 0, dropped), (b, c)
            want = torch.where(dropped, r_slot[ref].long(), r_slot[ref].long() + base[r_expert[ref].long()])
            assert torch.equal(slot[mine].long(), want), (b, c)
            some_dropped |= bool(dropped.any())
        assert torch.equal(l_aux[b:b + 1], r_aux), b
        base += r_kept.long()
        counts_sum += r_counts
    assert torch.equal(kept.long(), base) and torch.equal(counts, counts_sum)
    for c in range(top_k):                                      # the pad entries: routed nowhere
        e, s, w = (t[c * T:(c + 1) * T][pad] for t in (expert, slot, weight))
        assert bool((e == 0).all()) and bool((s == -1).all()) and bool((w == 0).all())
    if top_k == 1:                                              # slot_token inverts slot: the kept tokens of expert e, in slot order
        tok = torch.arange(T, device=dev)
        keep = slot >= 0
        assert torch.equal(slot_token[expert[keep].long(), slot[keep].long()].long(), tok[keep])
        for e in range(E):
            held = slot_token[e, :int(kept[e])].long()
            assert torch.equal(slot[held].long(), torch.arange(held.numel(), device=dev)) and bool((expert[held] == e).all())
    return some_dropped


@pytest.mark.parametrize("mode", CAPS)
@pytest.mark.parametrize("shape,E", CASES)
def test_top1_segments_are_the_unsegmented_op_per_segment(dev, shape, E, mode):
    lens, stride = SHAPES[shape]
    dropped = _check(dev, 1, list(lens), stride, E, _capacities(lens, E, 1, mode))
    if mode == "cf2.0" and shape != "one" and E == 2:
        assert not dropped                                  # ceil(n / 2 * 2.0) = n: no expert can overflow
    if mode in ("cf0.5", "one") and max(lens) > 8:
        assert dropped                                      # (or the case shows nothing)


@pytest.mark.parametrize("mode", CAPS)
@pytest.mark.parametrize("shape,E", CASES)
def test_top2_segments_are_the_unsegmented_op_per_segment(dev, shape, E, mode):
    lens, stride = SHAPES[shape]
    dropped = _check(dev, 2, list(lens), stride, E, _capacities(lens, E, 2, mode))
    if mode in ("cf0.5", "one") and max(lens) > 8:
        assert dropped


def test_a_batch_mate_takes_no_slot(dev):
    """What routing the padded batch as ONE pass gets wrong: segment 0 fills expert 0 to its capacity, and segment 1's tokens for expert 0
    are kept all the same, in slots behind segment 0's."""
    E, stride, lens, caps = 2, 8, [8, 5], [4, 3]
    gates = torch.tensor([[0.9, 0.1]], device=dev).repeat(2 * stride, 1).contiguous()
    gates[stride + 5:] = float("nan")
    expert, slot, weight, kept, counts, l_aux = ops.moe_route_top1_segments(gates, lens, stride, caps)
    assert slot.tolist() == [0, 1, 2, 3, -1, -1, -1, -1, 4, 5, 6, -1, -1, -1, -1, -1]
    assert kept.tolist() == [7, 0] and counts.tolist() == [13, 0] and expert.tolist() == [0] * 16
    one_pass = ops.moe_route_top1(torch.nan_to_num(gates, nan=0.5), sum(caps))
    assert one_pass[1].tolist()[stride:stride + 5] != [4, 5, 6, -1, -1]


def test_limits_are_error_codes(dev):
    """MP_ERR_SHAPE (-1) for a violated limit, MP_ERR_ARG (-5) for a null operand: refused on the host, before any launch."""
    L = _lib.lib()
    E, stride = 2, 16
    bufs = {}

    def call(top_k, lens, caps, slab_rows, stride=stride, E=E, null=None, n=None):
        n = len(lens) if n is None else n
        T = max(n, 1) * stride
        for name, shape, dt in (("gates", (T, E), torch.float32), ("logits", (T, E), torch.float32), ("expert", (2 * T,), torch.int32),
                                ("slot", (2 * T,), torch.int32), ("weight", (2 * T,), torch.float32), ("kept", (E,), torch.int32),
                                ("counts", (E,), torch.int64), ("l_aux", (max(n, 1),), torch.float32), ("slot_token", (E * 64,), torch.int32),
                                ("seg_kept", (max(n, 1) * E,), torch.int32), ("seg_counts", (max(n, 1) * E,), torch.int64)):
            bufs[name] = torch.zeros(shape, dtype=dt, device=dev)
        p = {k: (None if k == null else v.data_ptr()) for k, v in bufs.items()}
        lens_c, caps_c = (ctypes.c_int * 16)(*lens), (ctypes.c_int * 16)(*caps)
        lp = None if null == "seg_len" else ctypes.cast(lens_c, ctypes.c_void_p)
        cp = None if null == "seg_capacity" else ctypes.cast(caps_c, ctypes.c_void_p)
        if top_k == 1:
            return L.raw("mp_moe_route_top1_segments")(p["gates"], lp, cp, n, stride, E, slab_rows, p["expert"], p["slot"], p["weight"], p["kept"],
                                                       p["counts"], p["l_aux"], p["slot_token"], p["seg_kept"], p["seg_counts"], None)
        return L.raw("mp_moe_route_top2_segments")(p["gates"], p["logits"], lp, cp, n, stride, E, slab_rows, p["expert"], p["slot"], p["weight"],
                                                   p["kept"], p["counts"], p["l_aux"], p["seg_kept"], p["seg_counts"], None)

    for top_k in (1, 2):
        who = f"mp_moe_route_top{top_k}_segments"
        assert call(top_k, [16, 7], [8, 4], 12) == 0
        for bad in (dict(lens=[], caps=[], slab_rows=8, n=0), dict(lens=[4] * 9, caps=[2] * 9, slab_rows=18),
                    dict(lens=[16, 17], caps=[8, 8], slab_rows=16), dict(lens=[16, 0], caps=[8, 8], slab_rows=16),
                    dict(lens=[16, 7], caps=[8, 4], slab_rows=11), dict(lens=[16, 7], caps=[8, 4], slab_rows=12, E=9)):
            assert call(top_k, **bad) == -1 and who in L.last_error(), bad
        for null in ("gates", "seg_len", "seg_capacity", "expert", "slot", "weight", "kept", "counts", "l_aux", "seg_kept", "seg_counts") + \
                (("logits",) if top_k == 2 else ()):
            assert call(top_k, [16, 7], [8, 4], 12, null=null) == -5 and "null operand" in L.last_error(), null
    assert call(1, [16, 7], [8, 4], 12, null="slot_token") == 0            # optional
    assert call(1, [16, 7], [40, 40], 23) == 0 and call(1, [16, 7], [40, 40], 22) == -1      # a segment keeps at most its own tokens
    assert call(2, [16, 7], [40, 40], 46) == 0 and call(2, [16, 7], [40, 40], 45) == -1      # (top-2: two entries per token)
    torch.cuda.synchronize()
