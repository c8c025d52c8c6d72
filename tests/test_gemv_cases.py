"""CPU-only guard of tests/gemv_cases.py, the cases behind tests/test_gpu_gemv_edges.py: the operands are as exact as that file claims
(asserted, not trusted), the table reaches every route of the two entry points, every M of the shared form and both sides of every term
of the K-split predicate, and route() agrees with the sources it restates."""
import os
import re

import torch

import gemv_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _all_cases():
    out = []
    for w8 in (False, True):
        out += C.shared_cases(w8) + C.indexed_cases(w8)
    return out


def _assert_exact_dot(x, c, K, tag):
    """Every partial sum of x . c, in any association, is an integer below 2^24: max |c| * max |x| * K bounds them all."""
    assert int(c.abs().max()) <= 127 and float(x.float().abs().max()) <= 4 and bool((x.float() == x.float().round()).all()), tag
    assert int(c.abs().max()) * int(x.float().abs().max()) * K < 2 ** 24, tag


def test_grid_operands_are_what_they_claim():
    g = C.gen(1)
    for shape in ((1, 8), (5, 16), (3, 7, 520), (2, 130, 4112)):
        w, c, e = C.grid(g, *shape)
        assert w.shape == shape and c.shape == shape and e.shape == shape[:-1] and w.dtype == torch.bfloat16
        assert bool((c.abs().amax(-1) == 127).all()) and int(e.min()) >= -12 and int(e.max()) <= -5
        assert torch.equal(w.double(), c.double() * C.pow2(e).double().unsqueeze(-1))
        # the row-wise absmax format of such a row is (c, 2^e): absmax / 127 and 127 / absmax are powers of two
        absmax = w.float().abs().amax(-1)
        assert torch.equal(absmax / torch.tensor(127.0), C.pow2(e))
    x = C.ints(g, 8, 4096)
    assert set(x.float().unique().tolist()) == set(range(-4, 5))
    r = C.eighths(g, 8, 512)
    assert torch.equal((r.float() * 8).round() / 8, r.float()) and float(r.float().abs().max()) <= 8
    assert set(C.weights3(g, 256).tolist()) == set(C.SCALES)
    for s in C.SCALES:                                          # three mantissa bits
        assert s * 4 == int(s * 4) and 0.5 <= s < 2
    assert 127 * 4 * 8208 == 4169664 < 2 ** 24


def test_every_step_of_every_case_is_exact():
    """The dot product in any association, then a * alpha + bias (shared) or scale * bf16(a) (indexed): representable in fp32, so fma or
    mul + add, contracted or not, give the same number and the only roundings are the ones the references write out."""
    for case in _all_cases():
        o = C.operands(case)
        ws = o.c if not case.indexed else o.c[sorted(set(o.idx))]
        _assert_exact_dot(o.x, ws, case.K, case)
        assert C.is_f32(o.a), case
        if case.indexed:
            assert set(o.idx) <= set(range(C.E)) and 1 not in o.idx and len(o.idx) == case.M
            assert C.is_f32(o.row_scale.double().unsqueeze(-1) * C.bf(o.a).double()), case
            exact = torch.stack([o.x[m].double() @ o.w[o.idx[m]].double().T for m in range(case.M)])
            assert torch.equal(exact, o.a), case
        else:
            b = o.bias.double()
            assert float((b / C.pow2(o.e).double()).abs().max()) <= 1000 and torch.equal(b / C.pow2(o.e).double(), (b / C.pow2(o.e).double()).round())
            for alpha in (1.0, 0.5):
                assert C.is_f32(o.a * alpha) and C.is_f32(o.a * alpha + b), (case, alpha)
    for T, N, K in C.TOP2_DOWN:
        o = C.top2_operands(T, N, K, 700, swiglu=False)
        _assert_exact_dot(o.x, o.c, K, (T, N, K))
        dots = C.dot64_indexed(o.x, o.w, o.expert)
        assert C.is_f32(dots) and C.is_f32(o.weight.double().unsqueeze(-1) * C.bf(dots).double())
        # both products of a token and their sum are exact in float64, so the reference's one `.float()` per fma is the fma's rounding
        p = o.weight.double().unsqueeze(-1) * C.bf(dots).double()
        s = p[:T] + p[T:]
        assert torch.equal(s - p[:T], p[T:]) and torch.equal(s - p[T:], p[:T])
    for T, N, K in C.SWIGLU_INDEXED:
        o = C.top2_operands(T, N, K, 800, swiglu=True)
        _assert_exact_dot(o.x, o.c, K, (T, N, K))
    for w8 in (False, True):
        for term, left, right, rows, cols in C.predicate_pairs(w8):
            for o in (left, right):
                _assert_exact_dot(o.x, o.c, o.K, term)
                assert C.is_f32(o.a)
            assert torch.equal(left.a[:rows, :cols], right.a[:rows, :cols]), term
            assert torch.equal(left.res[:rows, :cols], right.res[:rows, :cols]) and torch.equal(left.e[:cols], right.e[:cols])
            assert bool((left.c.abs().amax(-1) == 127).all() and (right.c.abs().amax(-1) == 127).all())


def test_references_round_where_the_epilogues_round():
    """The float64 references against the same chains written with fp32 torch operations on the CPU (IEEE, uncontracted)."""
    for case in (C.shared_cases(False)[4], C.shared_cases(True)[6]):
        o = C.operands(case)
        a32 = o.a.float()
        for alpha in (1.0, 0.5):
            for act in (C.ACT_NONE, C.ACT_RELU):
                v = a32 * alpha + o.bias
                v = v.clamp_min(0) if act == C.ACT_RELU else v
                assert torch.equal(C.ref_shared(o.a, alpha, o.bias, act, None, True), v)
                assert torch.equal(C.ref_shared(o.a, alpha, o.bias, act, o.res, True), v + o.res.float())
                assert torch.equal(C.ref_shared(o.a, alpha, o.bias, act), v.to(torch.bfloat16))
                assert torch.equal(C.ref_shared(o.a, alpha, o.bias, act, o.res), (v.to(torch.bfloat16).float() + o.res.float()).to(torch.bfloat16))
        assert bool((C.ref_shared(o.a, 1.0, o.bias, C.ACT_RELU, None, True) == 0).any()), "ReLU clamps nothing in this case"
    o = C.operands(C.indexed_cases(False)[4])
    keep = C.keep_patterns(o.M)["first"]
    ref = C.ref_indexed(o.a, o.row_scale, o.res, keep)
    assert torch.equal(ref[0], o.res[0])
    for m in range(1, o.M):
        assert torch.equal(ref[m], (o.row_scale[m] * o.a[m].float().to(torch.bfloat16).float() + o.res[m].float()).to(torch.bfloat16))
    assert torch.equal(C.ref_indexed(o.a, None, None, keep)[0].view(torch.int16), torch.zeros(o.N, dtype=torch.int16))
    T, N, K = C.TOP2_DOWN[1]
    t = C.top2_operands(T, N, K, 700, swiglu=False)
    dots = C.dot64_indexed(t.x, t.w, t.expert)
    for name, slot in C.top2_patterns(T).items():
        y = dots.float().to(torch.bfloat16).float()
        acc = torch.zeros(T, N)
        for c in range(2):
            for tok in range(T):
                if slot[c * T + tok] >= 0:
                    acc[tok] = t.weight[c * T + tok] * y[c * T + tok] + acc[tok]      # the product is exact: this add is the fma's one rounding
        assert torch.equal(C.ref_top2_down(dots, t.weight, slot, t.res), (t.res.float() + acc).to(torch.bfloat16)), name
    assert torch.equal(C.ref_top2_down(dots, t.weight, [-1] * (2 * T), t.res), t.res)


def test_route_restates_the_two_entry_points():
    """The predicate text and the 4 + (M - 4) split occur once under csrc/, in the header both entry points dispatch through, and route() is
    that predicate, the indexed branch, then the split."""
    csrc = os.path.join(ROOT, "medplib_amd", "csrc")
    srcs = {name: open(os.path.join(csrc, name)).read() for name in sorted(os.listdir(csrc)) if name.endswith((".h", ".hip", ".cpp"))}
    predicate = r"act != ACT_SWIGLU_PAIR && N <= 4096 && K >= 4096 && \(w_index \|\| M == 1\)"
    for text in (predicate, r"\.M = M - 4"):                # (the second pass of the split; anchored, so another kernel may still write "M - 4")
        assert {name: len(re.findall(text, src)) for name, src in srcs.items() if re.search(text, src)} == {"gemv_forms.h": 1}, text
    assert "gemv_bf16.hip" in srcs and "gemv_w8.hip" in srcs
    for w8 in (False, True):
        assert C.route(1, 4096, 4096, False, False, w8) == ("ksplit", None)
        assert C.route(1, 4097, 4096, False, False, w8) == ("shared", (1,))
        assert C.route(1, 4096, 4088, False, False, w8) == ("shared", (1,))
        assert C.route(2, 4096, 4096, False, False, w8) == ("shared", (2,))
        assert C.route(2, 4096, 4096, True, False, w8) == ("ksplit", None)
        assert C.route(2, 4096, 4088, True, False, w8) == ("indexed", None)
        assert C.route(1, 4096, 4096, False, True, w8) == ("shared", (1,))
        assert C.route(3, 128, 4096, True, True, w8) == ("indexed", None)
        assert [C.route(M, 64, 512, False, False, w8)[1] for M in range(1, 9)] == [(1,), (2,), (3,), (4,), (4, 1), (4, 2), (4, 3), (4, 4)]


def test_table_reaches_every_route_and_every_listed_size():
    for w8 in (False, True):
        shared, indexed = C.shared_cases(w8), C.indexed_cases(w8)
        assert all(c.w8 == w8 and not c.indexed for c in shared) and all(c.w8 == w8 and c.indexed for c in indexed)
        assert len({c.seed for c in shared + indexed}) == len(shared + indexed)
        r_sh = [(c, C.route(c.M, c.N, c.K, False, False, w8)) for c in shared]
        r_ix = [(c, C.route(c.M, c.N, c.K, True, False, w8)) for c in indexed]
        assert {r[0] for _, r in r_sh} == {"shared", "ksplit"} and {r[0] for _, r in r_ix} == {"indexed", "ksplit"}
        assert {r[1] for _, r in r_sh if r[0] == "shared"} == {(1,), (2,), (3,), (4,), (4, 1), (4, 2), (4, 3), (4, 4)}
        forms = {"shared": [c for c, r in r_sh if r[0] == "shared"], "ksplit": [c for c, r in r_sh if r[0] == "ksplit"],
                 "indexed": [c for c, r in r_ix if r[0] == "indexed"], "ksplit_indexed": [c for c, r in r_ix if r[0] == "ksplit"]}
        want = {"shared": (C.N_ALL, C.K_SHARED[w8], range(1, 9)), "ksplit": (C.N_KSPLIT, C.K_KSPLIT[w8], (1,)),
                "indexed": (C.N_ALL, C.K_INDEXED[w8], C.M_INDEXED), "ksplit_indexed": (C.N_KSPLIT, C.K_KSPLIT[w8], C.M_INDEXED)}
        step = 1024 if w8 else 512
        for form, cases in forms.items():
            Ns, Ks, Ms = want[form]
            assert {c.N for c in cases} == set(Ns), (w8, form)
            assert {c.K for c in cases} == set(Ks), (w8, form)
            assert {c.M for c in cases} == set(Ms), (w8, form)
            assert any(c.N % 4 and c.K % step for c in cases), (w8, form, "ragged N never meets ragged K")
        assert all(c.K % (16 if w8 else 8) == 0 for c in shared + indexed)
        assert any(c.N < 4 for c in forms["shared"]) and any(c.N < 4 for c in forms["indexed"])
    both = C.both_types_cases()
    assert all(c.K % 16 == 0 and not c.w8 for c in both)
    assert {(c.indexed, c.M, c.N, c.K) for c in both} >= {(c.indexed, c.M, c.N, c.K) for c in C.shared_cases(True) + C.indexed_cases(True)}
    assert {C.route(c.M, c.N, c.K, c.indexed, False, False)[0] for c in both} == {"shared", "indexed", "ksplit"}
    # the SwiGLU forms, top-2 and the quantiser
    assert {M for M, N, K in C.SWIGLU_SHARED} == set(range(1, 9)) and {N for M, N, K in C.SWIGLU_SHARED} == set(C.N_SWIGLU)
    assert {T for T, N, K in C.SWIGLU_INDEXED} == set(C.TOKENS) and {N for T, N, K in C.SWIGLU_INDEXED} == set(C.N_SWIGLU)
    assert all(N % 64 == 0 and K % 16 == 0 for _, N, K in C.SWIGLU_SHARED + C.SWIGLU_INDEXED)
    assert {T for T, N, K in C.TOP2_DOWN} == set(C.TOKENS) and {N for T, N, K in C.TOP2_DOWN} == set(C.N_KSPLIT)
    assert {K for T, N, K in C.TOP2_DOWN} == {4096, 4104, 4608, 8, 520}
    assert C.QUANT_K == (16, 240, 256, 272) and C.QUANT_ROWS == (1, 3)


def test_predicate_pairs_differ_in_one_term_only():
    for w8 in (False, True):
        pairs = C.predicate_pairs(w8)
        assert [t for t, *_ in pairs] == ["N", "K", "M"]
        for i, (term, left, right, rows, cols) in enumerate(pairs):
            tl, tr = C.ksplit_terms(left.M, left.N, left.K, False), C.ksplit_terms(right.M, right.N, right.K, False)
            assert all(tl) and [a != b for a, b in zip(tl, tr)] == [j == i for j in range(3)], term
            assert C.route(left.M, left.N, left.K, False, False, w8)[0] == "ksplit"
            assert C.route(right.M, right.N, right.K, False, False, w8)[0] == "shared"
            others = {"N": (left.M == right.M, left.K == right.K), "K": (left.M == right.M, left.N == right.N),
                      "M": (left.N == right.N, left.K == right.K)}[term]
            assert all(others) and rows <= min(left.M, right.M) and cols <= min(left.N, right.N)
            assert right.K % (16 if w8 else 8) == 0
    assert (C.predicate_pairs(False)[1][2].K, C.predicate_pairs(True)[1][2].K) == (4088, 4080)


def test_keep_patterns_hold_every_drop_pattern():
    for M in C.M_INDEXED:
        pats = C.keep_patterns(M)
        assert len({tuple(p) for p in pats.values()}) == len(pats) and all(len(p) == M for p in pats.values())
        assert pats["none"] == list(range(M)) and (M == 1 or set(pats) == {"none", "first", "last", "all"})
        assert any(p[0] < 0 for p in pats.values()) and any(p[-1] < 0 and p[0] >= 0 for p in pats.values()) == (M > 1)
        assert any(all(s < 0 for s in p) for p in pats.values())
    kinds = set()
    for T in C.TOKENS:
        pats = C.top2_patterns(T)
        assert all(len(p) == 2 * T for p in pats.values()) and len(C.top2_experts(T)) == 2 * T and 1 not in C.top2_experts(T)
        for p in pats.values():
            kinds |= C.token_kinds(p)
        assert C.token_kinds(pats["none"]) == {"both"} and C.token_kinds(pats["all"]) == {"neither"}
        if T == 8:
            assert C.token_kinds(pats["mixed"]) == set(C.TOKEN_KINDS)
    assert kinds == set(C.TOKEN_KINDS)
    assert C.token_kinds(C.top2_patterns(1)["first"]) == {"second_only"} and C.token_kinds(C.top2_patterns(1)["last"]) == {"first_only"}
