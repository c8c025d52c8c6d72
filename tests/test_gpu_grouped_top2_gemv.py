"""The grouped top-2 expert GEMVs (mp_gemv_grouped_top2_gate_up_bf16 / mp_gemv_grouped_top2_down_bf16: one weight stream per expert) against the
per-entry pair (mp_gemv_top2_gate_up_bf16 / mp_gemv_top2_down_bf16) on the same arguments, bit for bit, and the down kernel against the float64
reference of tests/gemv_cases.py, which is exact on the grid operands.  No tolerance anywhere.

Guard bands as in tests/test_gpu_gemv_edges.py: every operand is a view into a larger arena — x, act and residual rows padded with NaN, the
outputs the corner of a sentinel arena whose guard rows and columns must not change, expert / slot / weight between poison entries.  The weight
arena here has a NaN matrix in FRONT of expert 0 and one BEHIND expert E - 1, so a read at expert index -1 or E shows as a NaN; experts no
entry names are NaN too.  All of it is ordinary allocated memory and every call satisfies the entry points' own preconditions."""
import functools
from types import SimpleNamespace

import pytest
import torch

import gemv_cases as C
from test_gpu_decode_top2 import _route_with_drops
from test_gpu_gemv_edges import NAN, _bits, _call, _dropped, _mid, _out_arena, _padded, _take

pytestmark = pytest.mark.gpu

GATE_UP = {False: "mp_gemv_top2_gate_up_bf16", True: "mp_gemv_grouped_top2_gate_up_bf16"}
DOWN = {False: "mp_gemv_top2_down_bf16", True: "mp_gemv_grouped_top2_down_bf16"}


def _valid(o):
    return [e for e in range(2 * o.T) if 0 <= o.expert[e] < o.E]


def _weights(o, dev):
    """[guard][E experts][guard], each [N + 1, K + 16] at a stride that is a multiple of 16 elements: NaN everywhere but the [N, K] corner of
    the experts some entry names -> (arena, address of expert 0, ldw, strideW); built once per operand set."""
    if "_arena" not in o.__dict__:
        E_, N, K = o.w.shape
        ldw = K + 16
        stride = ((N + 1) * ldw + 15) // 16 * 16
        a = torch.full(((E_ + 2) * stride,), NAN, dtype=torch.bfloat16)
        for s in sorted({o.expert[e] for e in _valid(o)}):
            a[(s + 1) * stride:(s + 1) * stride + (N + 1) * ldw].view(N + 1, ldw)[:N, :K] = o.w[s]
        d = a.to(dev)
        o._arena = (d, d[stride:].data_ptr(), ldw, stride)
    return o._arena


def _gate_up(dev, grouped, o, slot):
    """One gate|up launch of either kind on o (x [T, K], 2T entries) -> act [2T, N / 2]; the rows of entries that are dropped (or, grouped,
    name an expert outside [0, E)) must keep the sentinel."""
    _, W, ldw, strideW = _weights(o, dev)
    xd = _padded(o.x, 8, NAN).to(dev)
    y = _out_arena(2 * o.T, o.N // 2, False, dev)
    (ed, ep), (sd, sp) = _mid(o.expert, o.E + 7, torch.int32, dev), _mid(slot, -1, torch.int32, dev)
    _call(GATE_UP[grouped], xd.data_ptr(), xd.stride(0), W, ldw, strideW, y.data_ptr(), y.stride(0), ep, sp, o.T, o.N, o.K, *((o.E,) if grouped else ()))
    unwritten = sorted(set(_dropped(slot)) | (set(range(2 * o.T)) - set(_valid(o))))
    return _take(y, 2 * o.T, o.N // 2, False, ("gate_up", grouped, o.T, o.N, o.K, slot), unwritten=unwritten)


def _down(dev, grouped, o, slot, res):
    """One down launch of either kind on o (act [2T, K]; the act rows of entries that stream nothing are NaN) -> y [T, N]."""
    _, W, ldw, strideW = _weights(o, dev)
    x = o.x.clone()
    for e in set(_dropped(slot)) | (set(range(2 * o.T)) - set(_valid(o))):
        x[e] = NAN                                              # what the gate|up kernel leaves unwritten
    xd = _padded(x, 8, NAN).to(dev)
    rd = _padded(o.res, 8, NAN).to(dev) if res else None
    y = _out_arena(o.T, o.N, False, dev)
    (ed, ep), (sd, sp), (wd, wp) = (_mid(o.expert, o.E + 7, torch.int32, dev), _mid(slot, -1, torch.int32, dev), _mid(o.weight, NAN, torch.float32, dev))
    _call(DOWN[grouped], xd.data_ptr(), xd.stride(0), W, ldw, strideW, y.data_ptr(), y.stride(0), rd.data_ptr() if res else None,
          rd.stride(0) if res else 0, ep, sp, wp, o.T, o.N, o.K, *((o.E,) if grouped else ()))
    return _take(y, o.T, o.N, False, ("down", grouped, o.T, o.N, o.K, slot, res))


def _as_dropped(dev, o, slot):
    """(o', slot') for the per-entry kernels and the reference: the entries whose expert index lies outside [0, E) dropped (and given expert 0,
    which a dropped entry never reads)."""
    bad = set(range(2 * o.T)) - set(_valid(o))
    if not bad:
        return o, slot
    p = SimpleNamespace(**{k: v for k, v in o.__dict__.items() if k != "_arena"})
    p.expert = [0 if e in bad else x for e, x in enumerate(o.expert)]
    p._arena = _weights(o, dev)                                 # (the same arena: the experts o's VALID entries name)
    return p, [-1 if e in bad else s for e, s in enumerate(slot)]


def _check_gate_up(dev, o, slot, tag):
    po, pslot = _as_dropped(dev, o, slot)
    ref = _gate_up(dev, False, po, pslot)
    got = _gate_up(dev, True, o, slot)
    kept = [e for e in range(2 * o.T) if pslot[e] >= 0]
    assert torch.equal(_bits(got[kept]), _bits(ref[kept])), tag
    assert torch.equal(_bits(_gate_up(dev, True, o, slot)[kept]), _bits(got[kept])), (tag, "a second launch differs")


def _check_down(dev, o, slot, tag):
    po, pslot = _as_dropped(dev, o, slot)
    dots = C.dot64_indexed(o.x, o.w, po.expert)
    for res in (True, False):
        ref = _down(dev, False, po, pslot, res)
        got = _down(dev, True, o, slot, res)
        assert torch.equal(_bits(got), _bits(ref)), (tag, res)
        assert torch.equal(got, C.ref_top2_down(dots, o.weight, pslot, o.res if res else None)), (tag, res)
        assert torch.equal(_bits(_down(dev, True, o, slot, res)), _bits(got)), (tag, res, "a second launch differs")
        for t in range(o.T):
            if res and pslot[t] < 0 and pslot[o.T + t] < 0:
                assert torch.equal(_bits(got[t]), _bits(o.res[t])), (tag, t, "both choices dropped: the residual's bits")


@functools.lru_cache(maxsize=None)
def _operands(T, N, K, seed, swiglu):
    """The shared operands of gemv_cases (nobody writes to them) in a namespace of this file's own, which also holds the weight arena."""
    o = C.top2_operands(T, N, K, seed, swiglu)
    return SimpleNamespace(T=T, N=N, K=K, E=C.E, w=o.w, x=o.x, res=o.res, expert=o.expert, weight=o.weight)


@pytest.mark.parametrize("i", range(len(C.SWIGLU_INDEXED)))
def test_gate_up_equals_the_per_entry_kernel(dev, i):
    """Every SwiGLU case of the indexed table under every drop pattern: kept entries are the per-entry kernel's bits, dropped entries keep the
    sentinel, the guards are untouched, and a second launch gives the same bits."""
    T, N, K = C.SWIGLU_INDEXED[i]
    o = _operands(T, N, K, 800 + i, True)
    for name, slot in C.top2_patterns(T).items():
        _check_gate_up(dev, o, slot, (T, N, K, name))


@pytest.mark.parametrize("i", range(len(C.TOP2_DOWN)))
def test_down_equals_the_per_entry_kernel_and_the_float64_reference(dev, i):
    """Every top-2 down case (N in {3, 17, 66}; K with equal parts, a lane-0 tail, unequal parts and below one step; T in {1, 3, 8}) under every
    drop pattern, with and without a residual: the per-entry kernel's bits, equal to the float64 reference; the act rows of dropped entries are
    NaN and never read; a token with both choices dropped is the residual's bits."""
    T, N, K = C.TOP2_DOWN[i]
    o = _operands(T, N, K, 700 + i, False)
    for name, slot in C.top2_patterns(T).items():
        _check_down(dev, o, slot, (T, N, K, name))


def _layout(name):
    """-> (T, E, expert [2T], slot [2T]) of the other expert layouts."""
    if name == "single_choice_passes":          # every first choice on expert 0, every second on expert 2: two passes of four per expert, each of one choice
        return 8, 3, [0] * 8 + [2] * 8, list(range(16))
    if name == "four_plus_one":                 # expert 1: five kept entries (a pass of four, a pass of one); 0 and 3 the rest; 2 nobody
        expert = [1, 1, 1, 0, 3] + [0, 3, 0, 1, 1]
        assert expert.count(1) == 5 and 2 not in expert and all(expert[t] != expert[5 + t] for t in range(5))
        return 5, 4, expert, list(range(10))
    if name == "expert_out_of_range":           # entry 1 names expert E, entry 4 expert -1, both with kept slots
        expert = C.top2_experts(3)
        expert[1], expert[4] = 3, -1
        return 3, 3, expert, list(range(6))
    raise KeyError(name)


@pytest.mark.parametrize("name", ["single_choice_passes", "four_plus_one", "expert_out_of_range"])
def test_other_expert_layouts(dev, name):
    """Passes that hold entries of a single choice; an expert with a pass of four plus a pass of one beside an expert nobody names (NaN); and
    expert indices E and -1 with kept slots, which must be treated as dropped without a read outside the weight tensor (NaN on either side)."""
    T, E, expert, slot = _layout(name)
    for swiglu, (N, K) in ((True, (128, 1040)), (False, (17, 4104)), (False, (66, 520))):
        g = C.gen(1000 + len(name) + N)
        w, c, e = C.grid(g, E, N, K)
        o = SimpleNamespace(T=T, N=N, K=K, E=E, w=w, x=C.ints(g, T if swiglu else 2 * T, K), res=C.eighths(g, T, N), expert=expert,
                            weight=C.weights3(g, 2 * T))
        if swiglu:
            _check_gate_up(dev, o, slot, (name, N, K))
        else:
            _check_down(dev, o, slot, (name, N, K))


def test_the_pair_at_the_model_shape(dev):
    """d = 4096, ff = 11008, E = 3, B = 8, random bf16 weights, routing with capacity 3 (second choices of rows 3.. dropped, both choices of
    rows 6, 7): the grouped pair equals the per-entry pair, and the rows with both choices dropped are the residual."""
    from medplib_amd import ops
    d, ff, E, B = 4096, 11008, 3, 8
    gd = torch.Generator(device=dev).manual_seed(48)
    gu = (torch.randn((E, 2 * ff, d), generator=gd, device=dev) * 0.02).to(torch.bfloat16)
    down = (torch.randn((E, d, ff), generator=gd, device=dev) * 0.02).to(torch.bfloat16)
    h = torch.randn((B, d), generator=gd, device=dev).to(torch.bfloat16)
    x = torch.randn((B, d), generator=gd, device=dev).to(torch.bfloat16)
    expert, slot, weight, _, _, _ = _route_with_drops(B, E, 3, dev, torch.Generator().manual_seed(48))
    sl = slot.cpu()
    assert bool(((sl[:B] >= 0) & (sl[B:] < 0)).any()) and bool((sl[6:8] < 0).all() and (sl[B + 6:] < 0).all())
    act_ref = ops.gemv_top2_gate_up(h, gu, expert, slot)
    act = ops.gemv_grouped_top2_gate_up(h, gu, expert, slot)
    kept = slot >= 0
    assert torch.equal(act[kept], act_ref[kept])
    out_ref = ops.gemv_top2_down(act_ref, down, expert, slot, weight, x)
    out = ops.gemv_grouped_top2_down(act, down, expert, slot, weight, x)
    torch.cuda.synchronize()
    assert torch.equal(out, out_ref)
    assert torch.equal(out[6:8], x[6:8])
