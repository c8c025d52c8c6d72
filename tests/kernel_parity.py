"""Helpers shared by the kernel-level parity tests (test_gpu_train_kernels.py, test_gpu_glue_kernels.py, test_gpu_attention_edges.py,
test_gpu_row_kernels.py, test_gpu_f32_tail_kernels.py), the crafted MoE routing cases their CPU guard checks (test_kernel_coverage.py)
and the crafted row-kernel inputs (test_row_kernel_cases.py).  Plain torch on the CPU only: nothing here touches the GPU."""
import torch

U32 = 2.0 ** -24          # unit roundoff of fp32 (half an ulp, relative)
BF16_RTOL = 2 * 2.0 ** -8  # the suite's allowance for one bf16 output rounding (test_gpu_trunk_kernels._report)
FP32_EPS = 1.1920929e-07


def bf(x):
    """Round to bf16 and come back as float32: the value a bf16 tensor holds."""
    return x.to(torch.bfloat16).float()


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def assert_bits(name, got, ref):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, f"{name}: shape {tuple(g.shape)} != {tuple(r.shape)}"
    n = int((g != r).sum())
    print(f"{name}: {n}/{g.numel()} elements differ in their bits")
    assert torch.equal(g, r), f"{name}: {n}/{g.numel()} elements differ in their bits"


def report(name, got, ref, rtol, atol):
    """|got - ref| <= atol + rtol |ref| on every element (atol a number or a tensor of ref's shape); prints the worst ratio first."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    err = (got - ref).abs()
    tol = rtol * ref.abs() + atol
    bad = ~(err <= tol)                                  # NaN counts as bad
    ratio = err / tol.clamp_min(1e-300)
    msg = (f"{name}: max|err|={err.max().item():.4e}, max err/tol={ratio.max().item():.3f}, ref absmax={ref.abs().max().item():.4e}, "
           f"bad={int(bad.sum())}/{bad.numel()}")
    print(msg)
    assert not bad.any(), msg


# ---------------------------------------------------------------------------------------------------------------------------------
# DeepSpeed-style routing restated on the CPU (first-come capacity, no random draws), used to PROVE that the crafted cases hold
# every drop pattern before they go to the GPU; the GPU test then requires the project's router to return exactly these arrays.
def route_top1_cpu(gates, cap):
    T, E = gates.shape
    expert = gates.argmax(1).to(torch.int32)             # first maximum (the kernel takes a strictly larger value only)
    slot = torch.full((T,), -1, dtype=torch.int32)
    seen = [0] * E
    for t in range(T):
        e = int(expert[t])
        if seen[e] < cap:
            slot[t] = seen[e]
        seen[e] += 1
    weight = gates[torch.arange(T), expert.long()].clone()
    return expert, slot, weight, torch.tensor(seen, dtype=torch.int64)


def route_top2_cpu(gates, logits, cap):
    """-> (expert [2T], slot [2T], weight [2T] in float64 (the kept pair renormalised, denominator clamped at fp32 eps),
    first-choice counts [E]).  Second choices queue behind ALL first choices of their expert."""
    T, E = gates.shape
    e1 = gates.argmax(1)
    masked = logits.clone()
    masked[torch.arange(T), e1] = float("-inf")
    e2 = masked.argmax(1)
    tot1 = torch.bincount(e1, minlength=E)
    slot = torch.full((2 * T,), -1, dtype=torch.int32)
    s1, s2 = [0] * E, [int(v) for v in tot1]
    for t in range(T):
        a, b = int(e1[t]), int(e2[t])
        if s1[a] < cap:
            slot[t] = s1[a]
        s1[a] += 1
        if s2[b] < cap:
            slot[T + t] = s2[b]
        s2[b] += 1
    g = gates.double()
    g1 = torch.where(slot[:T] >= 0, g[torch.arange(T), e1], torch.zeros(T, dtype=torch.float64))
    g2 = torch.where(slot[T:] >= 0, g[torch.arange(T), e2], torch.zeros(T, dtype=torch.float64))
    den = (g1 + g2).clamp_min(FP32_EPS)
    return torch.cat([e1, e2]).to(torch.int32), slot, torch.cat([g1 / den, g2 / den]), tot1.to(torch.int64)


def _gates_for(pairs, E, seed):
    """fp32 (logits, gates) whose first / second choices are the given (e1, e2) pairs: 2 on the first, 1 on the second, -1 elsewhere,
    plus a small seeded jitter so that no two gate values are equal."""
    g = torch.Generator().manual_seed(seed)
    T = len(pairs)
    logits = torch.full((T, E), -1.0) + 0.05 * torch.rand(T, E, generator=g)
    for t, (a, b) in enumerate(pairs):
        logits[t, a] += 3.0
        if b != a:
            logits[t, b] += 2.0
    logits = logits.float()
    return logits, torch.softmax(logits, dim=1)


def moe_cases():
    """[(name, E, capacity, logits, gates)].  Token order matters: capacity is first-come."""
    cases = []
    # E = 4, capacity 6: 13 first choices on expert 0 (over capacity), expert 1's second choices fill up, expert 3 never named
    pairs = [(0, 1)] * 10 + [(1, 0)] * 3 + [(0, 2)] * 3 + [(2, 1)] * 2
    cases.append(("e4_all_patterns", 4, 6) + _gates_for(pairs, 4, 1))
    # E = 2, capacity 3
    cases.append(("e2_tight", 2, 3) + _gates_for([(0, 1)] * 5 + [(1, 0)] * 3, 2, 2))
    # E = 8, capacity 4, experts 6 and 7 never named; a seeded mix over experts 0..5
    g = torch.Generator().manual_seed(3)
    a = torch.randint(0, 6, (48,), generator=g)
    b = (a + 1 + torch.randint(0, 5, (48,), generator=g)) % 6
    cases.append(("e8_mixed", 8, 4) + _gates_for(list(zip(a.tolist(), b.tolist())), 8, 3))
    # nothing dropped: capacity = every entry
    cases.append(("e4_no_drops", 4, 64) + _gates_for([(t % 4, (t + 1) % 4) for t in range(32)], 4, 4))
    return cases


def drop_patterns(slot, T):
    """The set of per-token patterns in a top-2 slot array."""
    k1, k2 = slot[:T] >= 0, slot[T:] >= 0
    out = set()
    if bool((k1 & k2).any()): out.add("none")
    if bool((~k1 & k2).any()): out.add("first_only")
    if bool((k1 & ~k2).any()): out.add("second_only")
    if bool((~k1 & ~k2).any()): out.add("both")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Attention parity (tests/test_gpu_attention_edges.py): readout values, a float64 reference that also returns P, and per-element
# bounds derived from the kernels' rounding points.
#
# What the forward kernels round (attention.hip: attn_fwd2_kernel, attn_fwd_kernel, attn_decode_kernel -- the same in all three):
#   scores in fp32 (MFMA / fmaf chain over D), p = exp(s - m) in fp32, the normaliser l = sum(p) from the UNROUNDED p in fp32,
#   p rounded to bf16 before the PV product, fp32 PV accumulation, (o / l) rounded to bf16 on the store.
# With u = 2^-8 (unit roundoff of bf16) and U32 = 2^-24:
#   |got - ref| <= c * (P @ |V|),     c = 2u + u^2 + 2 (E_s + E_exp) + (2 Sk + 3 T + 2) U32 [+ the decode merge]
#     u        p -> bf16 (relative, per key, so the numerator moves by at most u * sum p_k |v_k|)
#     u + u^2  the bf16 store of a value that is already off by the other terms
#     E_s      = (D + 5) U32 A, A = max over (query, key) of scale * sum_d |q_d| |k_d|: fp32 accumulation of D products (<= D U32 A
#                whatever the order), the multiplication by the scale (1 rounding on |s| <= A), the subtraction of the row max and
#                __expf's multiplication by log2(e) (1 rounding each on |s - m| <= 2A).  An ABSOLUTE error of the exponent, so a
#                RELATIVE one of p; it moves the numerator and the normaliser, hence the factor 2
#     E_exp    = 2^-22: v_exp_f32 is taken to be good to 1 ulp (2^-23 relative; the ISA manual's figure); the second ulp covers the
#                v_log_f32 / __expf wrappers' own last operation.  ASSUMPTION about the device math functions, see the record
#     Sk U32   the fp32 sum of Sk terms, once for l and once for the PV accumulation (any order: <= (n - 1) U32 relative to sum |.|)
#     3 T U32  T = ceil(Sk / 32) key tiles at most (the MP_ATTN_KT=32 form): per tile one rescale factor (an exp of a value that
#              is exact up to E_s, already counted), one multiply of the accumulator and one of l
#     2 U32    1 / l and the product with it
#   decode: every split leaves (max, sum, o); the merge adds 2 (E_exp + (NS + 1) U32) for w = exp(m_s - M) and the two NS-term sums,
#           and 48 U32 for the block-wide sums (32 row partials at most + the wave / block reduction tree)
# All of it is 1e-5 .. 1e-4 against 2u = 7.8e-3 unless the scores themselves are large (A ~ 100: E_s ~ 8e-4).
# Absolute floor: p below 2^-126 is flushed, so up to Sk keys may each lose 2^-126 max|V|.  Nothing else.
U_BF16 = 2.0 ** -8
E_EXP = 2.0 ** -22
LOG2E = 1.4426950408889634


def readout_values(S, D, kind):
    """[S, D] one-hot rows, exact in bf16: 'mod' -> V[k] = e_{k mod D} (column c of the output is the probability mass of the keys
    = c mod D; for S <= D the whole P matrix), 'div' -> V[k] = e_{(k // D) mod D} (mass per block of D consecutive keys)."""
    k = torch.arange(S)
    col = k % D if kind == "mod" else (k // D) % D
    v = torch.zeros(S, D)
    v[k, col] = 1.0
    return v


def attn_allowed(B, Sq, Sk, causal, key_valid):
    """bool [B, 1, Sq, Sk]: key kj is admissible for query qi.  The causal mask is top-left aligned (kj <= qi), as in oracle.ops.attention."""
    ok = torch.ones(B, 1, Sq, Sk, dtype=torch.bool)
    if causal:
        ok = ok & torch.ones(Sq, Sk, dtype=torch.bool).tril()[None, None]
    if key_valid is not None:
        ok = ok & key_valid.bool()[:, None, None, :]
    return ok


def attn_probs64(q, k, allowed, scale):
    """float64 softmax of the masked scaled scores.  q [B,Sq,H,D], k [B,Sk,H,D] float64 (may require grad).
    -> (P [B,H,Sq,Sk], lse2 [B,H,Sq] = log2 of the row's sum of exp).  A masked score gets zero weight; a row with no admissible
    key gets P = 0 and lse2 = +inf (what 2^(s - lse2) = 0 needs), never NaN, also under autograd."""
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    s = s.masked_fill(~allowed, float("-inf"))
    m = s.detach().amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    dead = l.detach() == 0
    p = e / torch.where(dead, torch.ones_like(l), l)
    lse2 = torch.where(dead, torch.full_like(l, float("inf")), (m + torch.log(torch.where(dead, torch.ones_like(l), l))) * LOG2E)
    return p, lse2.squeeze(-1)


def attn_score_mag(q, k, scale):
    """A of the derivation: max over (query, key) of scale * sum_d |q_d| |k_d|."""
    return float(torch.einsum("bqhd,bkhd->bhqk", q.double().abs(), k.double().abs()).max()) * scale


def attn_fwd_c(D, Sk, A, splits=0):
    """The constant c of |got - ref| <= c (P @ |V|); splits > 0: the decode kernel with that many splits."""
    e_s = (D + 5) * U32 * A
    tiles = (Sk + 31) // 32
    c = 2 * U_BF16 + U_BF16 ** 2 + 2 * (e_s + E_EXP) + (2 * Sk + 3 * tiles + 2) * U32
    if splits:
        c += 2 * (E_EXP + (splits + 1) * U32) + 48 * U32
    return c


def attn_fwd_floor(Sk, vmax):
    return Sk * 2.0 ** -126 * vmax


def attn_lse2_tol(D, Sk, A, lse2_abs):
    """lse2 = m + log2(l) in the log2 domain.  m cancels (m + log2 sum 2^(s - m) = log2 sum 2^s exactly in m), so what is left is the
    scores' own error E_s and the relative error of l (E_exp, the Sk-term sum, the per-tile rescale), both times log2(e); v_log_f32,
    taken good to 2 ulp AT THE LARGEST value log2(l) can have (l <= Sk: 4 U32 max(1, log2 Sk), assumption, see the record); and the
    final fp32 addition (U32 |lse2|, doubled for the rounding of m itself)."""
    import math
    e_s = (D + 5) * U32 * A
    tiles = (Sk + 31) // 32
    return LOG2E * (e_s + E_EXP + (Sk + 3 * tiles) * U32) + 4 * U32 * max(1.0, math.log2(max(Sk, 2))) + 2 * U32 * lse2_abs


def ratio_check(name, got, ref, bound, worst=None, group=None):
    """err / bound on every element (bound a float64 tensor, zero where the reference is exactly zero by construction: there the
    result has to be exact).  Prints the worst ratio BEFORE asserting and files it under worst[group]."""
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.detach().double()
    err = (got - ref).abs()
    fin = bool(torch.isfinite(got).all())
    ratio = torch.where(err <= bound, err / bound.clamp_min(1e-300), torch.full_like(err, float("inf")))
    ratio = torch.where((err == 0), torch.zeros_like(err), ratio)
    r = float(ratio.max()) if fin else float("inf")
    if worst is not None:
        worst[group or name] = max(worst.get(group or name, 0.0), r)
    i = int(ratio.flatten().argmax())
    msg = (f"{name}: worst err/bound={float((err / bound.clamp_min(1e-300)).flatten()[i]):.3f} (err {float(err.flatten()[i]):.3e}, bound "
           f"{float(bound.flatten()[i]):.3e}, ref {float(ref.flatten()[i]):.3e}, flat index {i}), finite={fin}")
    print(msg)
    assert fin and r <= 1.0, msg
    return r


# Backward (attention_bwd.hip: attn_bwd_kernel).  Rounding points: s and dP = dO V^T in fp32 (MFMA); P = 2^(s c2 - L) in fp32 with the
# forward's L; delta = sum_d dO O in fp32 from the forward's bf16 O; dS = P (dP - delta) formed in fp32 from the UNROUNDED P; P -> bf16 for
# dV, dS -> bf16 for dQ / dK; fp32 accumulation; bf16 stores (dQ, dK after the multiplication by the scale).  With u = 2^-8:
#   eps_P  = E_s + E_exp + ln2 * tol(lse2)                              relative error of the fp32 P
#   tol_dV = (2u + u^2 + eps_P + Sq U32) (P^T @ |dO|)
#   E_delta= sum_d |dO_d| c_fwd (P @ |V|)_d + (D + 1) U32 sum_d |dO_d O_d|    the O it reads is the forward's OUTPUT: it carries the forward's
#            whole error c_fwd (P @ |V|) >= 2u |O|, not only the store rounding u |O| (this term is larger than u sum |dO O|)
#   eps_dP = (D + 1) U32 (|dO| @ |V|^T)
#   inner  = eps_P |dS| + P (eps_dP + E_delta + U32 (|dP| + |delta|))
#   E_dS   = u (|dS| + inner) + inner           (no u |dP - delta| term: P is not rounded before the product, the kernel keeps it in fp32)
#   tol_dQ = scale (1 + u) (E_dS @ |K| + Sk U32 (|dS| @ |K|)) + (u + U32) |dQ|,   tol_dK the same with E_dS^T, |Q|, Sq.
def attn_bwd_ref_and_tols(q, k, v, d_out, allowed, scale, c_fwd, lse_tol, A):
    """q,k,v [B,S,H,D], d_out [B,Sq,H*D]: float tensors holding bf16 values.  Reference = float64 autograd of attn_probs64 @ v.
    -> dict(dq, dk, dv, tol_dq, tol_dk, tol_dv) in float64, [B,S,H,D]."""
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    q64, k64, v64 = [t.double().clone().requires_grad_(True) for t in (q, k, v)]
    g = d_out.double().reshape(B, Sq, H, D)
    P, _ = attn_probs64(q64, k64, allowed, scale)
    o = torch.einsum("bhqk,bkhd->bqhd", P, v64)
    o.backward(g)
    P, o = P.detach(), o.detach()
    u = U_BF16
    eps_p = (D + 5) * U32 * A + E_EXP + 0.6931471805599453 * lse_tol
    dP = torch.einsum("bqhd,bkhd->bhqk", g, v64.detach())
    delta = (g * o).sum(-1).permute(0, 2, 1)[..., None]                       # [B,H,Sq,1]
    dS = P * (dP - delta)
    pv_abs = torch.einsum("bhqk,bkhd->bqhd", P, v64.detach().abs())
    e_delta = (c_fwd * (g.abs() * pv_abs).sum(-1) + (D + 1) * U32 * (g * o).abs().sum(-1)).permute(0, 2, 1)[..., None]
    eps_dp = (D + 1) * U32 * torch.einsum("bqhd,bkhd->bhqk", g.abs(), v64.detach().abs())
    inner = eps_p * dS.abs() + P * (eps_dp + e_delta + U32 * (dP.abs() + delta.abs()))
    e_ds = u * (dS.abs() + inner) + inner
    ka, qa = k64.detach().abs(), q64.detach().abs()
    tiny = 2.0 ** -120
    tol_dq = scale * (1 + u) * (torch.einsum("bhqk,bkhd->bqhd", e_ds, ka) + Sk * U32 * torch.einsum("bhqk,bkhd->bqhd", dS.abs(), ka)) \
        + (u + U32) * q64.grad.abs() + tiny
    tol_dk = scale * (1 + u) * (torch.einsum("bhqk,bqhd->bkhd", e_ds, qa) + Sq * U32 * torch.einsum("bhqk,bqhd->bkhd", dS.abs(), qa)) \
        + (u + U32) * k64.grad.abs() + tiny
    tol_dv = (2 * u + u * u + eps_p + Sq * U32) * torch.einsum("bhqk,bqhd->bkhd", P, g.abs()) + tiny
    return {"dq": q64.grad, "dk": k64.grad, "dv": v64.grad, "tol_dq": tol_dq, "tol_dk": tol_dk, "tol_dv": tol_dv}


# ---------------------------------------------------------------------------------------------------------------------------------
# Row, elementwise and fp32 tail kernels (tests/test_gpu_row_kernels.py, tests/test_gpu_f32_tail_kernels.py) and the CPU guard of
# their crafted inputs (tests/test_row_kernel_cases.py).  u = U_BF16 = 2^-8, U32 = 2^-24.  The device math functions (rsqrtf, sqrtf,
# the fp32 division, expf, __expf, erff, v_rcp_f32) are ASSUMED good to 2 ulp = 4 U32 (profiles/kernel_parity_tests.md); everything
# else in the bounds below counts roundings read off the kernels.
ULP2 = 4 * U32
CANARY = -7.5            # exact in bf16 and fp32; no kernel here produces a whole band of it


def gen(seed):
    return torch.Generator().manual_seed(seed)


def canary_view(rows, cols, ld, dtype, dev, lead=8):
    """(whole, view): a [rows, cols] view with row stride ld inside a buffer filled with CANARY, `lead` elements in front of the
    first row and a whole spare row behind the last one (lead a multiple of 8 keeps 16-byte alignment for bf16)."""
    whole = torch.full((lead + (rows + 1) * ld,), CANARY, dtype=dtype, device=dev)
    return whole, whole[lead:lead + rows * ld].view(rows, ld)[:, :cols]


def canary_intact(name, whole, rows, cols, ld, lead=8):
    """Everything of `whole` outside the [rows, cols] view still holds CANARY's bits."""
    w = whole.detach().cpu()
    keep = torch.ones(w.numel(), dtype=torch.bool)
    keep[lead:lead + rows * ld].view(rows, ld)[:, :cols] = False
    ref = torch.full_like(w, CANARY)
    n = int((bits(w)[keep] != bits(ref)[keep]).sum())
    print(f"{name}: {n}/{int(keep.sum())} canary elements changed")
    assert n == 0, f"{name}: {n} elements outside the output view were written"


def strided_in(t, ld, dev, lead=8):
    """The CPU tensor t [rows, cols] on the device as a view with row stride ld (CANARY in the gaps)."""
    whole, v = canary_view(t.shape[0], t.shape[1], ld, t.dtype, dev, lead)
    v.copy_(t.to(dev))
    return v


def bf16_ulp(x):
    """Spacing of bf16 at |x| (float64 tensor): 2^(e - 7), the subnormal spacing 2^-133 below 2^-126."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 7)


def bf16_flip_slack(t64, rel):
    """(bf16(t64) as float64, slack): slack = the distance between the two bf16 values that t64 (1 +- rel) round to: zero unless t64 is
    within rel |t64| of a rounding boundary, where a kernel whose fp32 value is off by that much may land on the neighbour."""
    lo, hi = bf((t64 * (1 - rel)).float()).double(), bf((t64 * (1 + rel)).float()).double()
    return bf(t64.float()).double(), (hi - lo).abs()


# RMSNorm (rmsnorm_bf16_kernel), HF order: t = bf16(x * rs), y = bf16(w * t).
#   ss = sum x^2: dim products and a sum of dim terms in any order: relative (dim + 1) U32 (all terms >= 0); / dim and + eps: 2 U32;
#   rsqrtf halves the relative error of its argument and adds ULP2: e_rs = ((dim + 3) / 2 + 4) U32; x * rs: one more U32.
#   Where x rs64 is within (e_rs + U32) of a bf16 rounding boundary, t may be the neighbouring bf16 value (bf16_flip_slack); elsewhere
#   t is the reference's.  y = bf16(fl32(w t)): u |w t| (1 + U32) + U32 |w t| <= (u + 2 U32) |w t|.
#   bound = (u + 2 U32) |w t_ref| + (1 + u) |w| slack
def rmsnorm_ref(x, w, eps):
    """x bf16 [rows, dim], w fp32 [dim] (CPU) -> (ref float64 = w * bf16(x rs), bound)."""
    x64, w64 = x.double(), w.double()
    dim = x.shape[-1]
    rs = torch.rsqrt((x64 * x64).mean(-1, keepdim=True) + eps)
    e_rs = ((dim + 3) / 2 + 4) * U32
    t, slack = bf16_flip_slack(x64 * rs, e_rs + U32)
    ref = w64 * t
    return ref, (U_BF16 + 2 * U32) * ref.abs() + (1 + U_BF16) * w64.abs() * slack


# LayerNorm.  Shared first-order analysis of y = (x - mean) rs w + b with fp32 statistics in two passes; `depth` = the longest chain
# of additions one element goes through in the kernel's sum (lane-sequential part + 6 shuffle levels [+ the waves of the block form]),
# so |fl(sum) - sum| <= depth U32 sum|.| whatever the values; sum_exact=True (inputs whose every partial sum is exactly representable:
# the offset and constant rows, proved by tests/test_row_kernel_cases.py) leaves only the division's rounding.
#   dm   = depth U32 mean|x| + U32 |mean|                                 error of the mean
#   d    = x - mean: |err| <= dm + U32 |d|
#   dvar = 2 mean|d| dm + dm^2 + (depth + 3) U32 var                      (d^2: 2 |d| err + err^2; dim products, the sum, the division)
#   e_rs = dvar / (2 (var + eps)) + U32 + e_root     (+ eps: one rounding; the root: `e_root` = ULP2 for rsqrtf, 2 ULP2 for 1 / sqrtf)
#   E    = |w| rs (dm + U32 |d|) + |d rs w| (e_rs + 3 U32) + 2 U32 (|d rs w| + |b|)       error of the fp32 value before the store
def layernorm_ref(x, w, b, eps, depth, sum_exact=False, e_root=ULP2):
    """x [rows, dim] (any float dtype, CPU), w, b fp32 or None -> dict(y, mean, rstd, E, dm, e_rs) in float64."""
    x64 = x.double()
    w64 = w.double()
    b64 = torch.zeros_like(w64) if b is None else b.double()
    mean = x64.mean(-1, keepdim=True)
    d = x64 - mean
    var = (d * d).mean(-1, keepdim=True)
    rs = torch.rsqrt(var + eps)
    dm = (0.0 if sum_exact else depth * U32) * x64.abs().mean(-1, keepdim=True) + U32 * mean.abs()
    dvar = 2 * d.abs().mean(-1, keepdim=True) * dm + dm * dm + (depth + 3) * U32 * var
    e_rs = dvar / (2 * (var + eps)) + U32 + e_root
    core = (d * rs * w64).abs()
    E = w64.abs() * rs * (dm + U32 * d.abs()) + core * (e_rs + 3 * U32) + 2 * U32 * (core + b64.abs())
    return {"y": d * rs * w64 + b64, "mean": mean.squeeze(-1), "rstd": rs.squeeze(-1), "E": E, "dm": dm.squeeze(-1), "e_rs": e_rs.squeeze(-1)}


def layernorm_bf16_bound(r):
    """The bf16 store of a value that is off by E: u (|y| + E) + E."""
    return U_BF16 * (r["y"].abs() + r["E"]) + r["E"]


LN_BF16_DEPTH = 32 + 6 + 4      # <= 4 chunks of 8 per lane, 6 shuffle levels, 4 waves summed in order (the block form)


def ln_f32_depth(dim):
    return -(-dim // 64) + 6


def offset_rows_bf16(rows, dim, seed):
    """Rows with mean ~100 and a spread of one bf16 step (0.5 at 100): values in {99.5, 100, 100.5}.  Every partial sum is a multiple
    of 0.5 below 2^23, hence exact in fp32 in any order."""
    return (100.0 + 0.5 * (torch.randint(0, 3, (rows, dim), generator=gen(seed)) - 1).float()).bfloat16()


def offset_rows_f32(rows, dim, seed):
    """fp32 rows with mean 1e3 and spread 1e-2."""
    return (1e3 + 1e-2 * torch.randn(rows, dim, generator=gen(seed), dtype=torch.float64)).float()


# LayerNorm backward (ln_bwd_f32_kernel) from the kernel's own fp32 mean / rstd (the reference reads the same values):
#   xh = (x - mu) rs: 2 U32 |xh|; g = dy w: U32 |g|; sg = mean(g), sgx = mean(g xh): depth-long sums
#   dsg = (depth + 2) U32 mean|g|, dsgx = (depth + 5) U32 mean|g xh|
#   dx = rs (g - sg - xh sgx): bound = rs (dsg + |xh| dsgx + 6 U32 (|g| + |sg| + |xh sgx|)) + U32 |dx|
def layernorm_bwd_ref(dy, x, w, mean, rstd):
    dy64, x64, w64 = dy.double(), x.double(), w.double()
    dim = x.shape[-1]
    depth = ln_f32_depth(dim)
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    xh = (x64 - mu) * rs
    g = dy64 * w64
    sg, sgx = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    dx = rs * (g - sg - xh * sgx)
    dsg = (depth + 2) * U32 * g.abs().mean(-1, keepdim=True)
    dsgx = (depth + 5) * U32 * (g * xh).abs().mean(-1, keepdim=True)
    bound = rs * (dsg + xh.abs() * dsgx + 6 * U32 * (g.abs() + sg.abs() + (xh * sgx).abs())) + U32 * dx.abs()
    # dw / db (ln_bwd_wb_f32_kernel): ceil(rows / 16) sequential terms per wave, 16 partials in order, the += : chain length below
    rows = x.shape[0]
    chain = -(-rows // 16) + 16 + 1
    tw, tb = (dy64 * xh).sum(0), dy64.sum(0)
    bw = (chain + 3) * U32 * (dy64 * xh).abs().sum(0)
    bb = chain * U32 * dy64.abs().sum(0)
    return {"dx": dx, "dx_bound": bound, "dw": tw, "dw_bound": bw, "db": tb, "db_bound": bb}


# Softmax forward (softmax_fwd_f32_kernel): p = expf(s x - m) / sum.  A = max |s x|.
#   exponent: fl(s x) and m = the largest fl(s x) are each off by U32 A, the subtraction by U32 * 2A: absolute 4 U32 A = relative e_s
#   of p; expf ULP2; the sum of depth-long chains; 1 / sum ULP2; the product U32.  The error of the normaliser is common to the row.
#   c = 2 (e_s + ULP2) + (depth + 1) U32 + ULP2 + U32;  floor 2^-125: a term or a result below 2^-126 may be flushed
def softmax_ref(x, scale):
    x64 = x.double() * scale
    p = torch.softmax(x64, -1)
    fin = torch.where(torch.isfinite(x64), x64, torch.zeros_like(x64))
    A = fin.abs().amax(-1, keepdim=True)
    c = 2 * (4 * U32 * A + ULP2) + (ln_f32_depth(x.shape[-1]) + 2) * U32 + ULP2
    bound = torch.where(p > 0, c * p + 2.0 ** -125, torch.zeros_like(p))
    return p, bound, c.squeeze(-1)


# Softmax backward: dx = s p (dp - sum(p dp)):  the sum: (depth + 1) U32 sum|p dp|; the difference and two products: 3 roundings;
# floor 2^-125 where p > 0: a product below 2^-126 is subnormal or flushed (p = 0 gives an exact zero)
def softmax_bwd_ref(p, dp, scale):
    p64, dp64 = p.double(), dp.double()
    s = (p64 * dp64).sum(-1, keepdim=True)
    ds = (ln_f32_depth(p.shape[-1]) + 1) * U32 * (p64 * dp64).abs().sum(-1, keepdim=True)
    dx = scale * p64 * (dp64 - s)
    return dx, abs(scale) * p64 * (ds + 2 * U32 * (dp64.abs() + s.abs())) + 3 * U32 * dx.abs() + 2.0 ** -125 * (p64 > 0)


def softmax_case(kind, rows, cols, seed):
    g = gen(seed)
    if kind == "random":
        return 3 * torch.randn(rows, cols, generator=g)
    if kind == "equal":
        return torch.full((rows, cols), 1.25) * torch.arange(1, rows + 1).float()[:, None]
    if kind == "spread":            # +-1e4: all but the few entries next to the maximum underflow
        x = (torch.rand(rows, cols, generator=g) * 2 - 1) * 1e4
        x[:, 0] = 1e4
        x[:, -1] = -1e4 if cols > 1 else 1e4
        return x
    if kind == "neginf":            # every other entry -inf beside finite ones (entry 0 stays finite)
        x = torch.randn(rows, cols, generator=g)
        x[:, 1::2] = float("-inf")
        return x
    raise ValueError(kind)


# exact erf GELU in fp32 (gelu_erf): y = 0.5 x (1 + erff(z)), z = fl(x * fl(1/sqrt2)).
#   erf: ULP2 |erf| + 2 U32 |z| erf'(z) (the constant's and the product's rounding of the argument);  1 + erf: U32 |1 + erf|
#   y: 0.5 |x| (that) + 2 U32 |y|.  For x << 0 the sum 1 + erf cancels: the bound there is absolute, ~ |x| ULP2 / 2.
def _erf_parts(x64):
    z = x64 * 0.7071067811865476
    erf = torch.erf(z)
    derf = 1.1283791670955126 * torch.exp(-z * z)
    e_sum = ULP2 * erf.abs() + 2 * U32 * z.abs() * derf + U32 * (1 + erf).abs()
    return erf, e_sum


def gelu_ref(x, dv=None):
    """float64 GELU of x and its bound; dv = an error the INPUT already carries (the sgemm epilogue): |gelu'| <= 1.13."""
    x64 = x.double()
    erf, e_sum = _erf_parts(x64)
    y = 0.5 * x64 * (1 + erf)
    bound = 0.5 * x64.abs() * e_sum + 2 * U32 * y.abs()
    if dv is not None:
        bound = bound + 1.13 * dv * (1 + ULP2)
    return y, bound


# GELU derivative (gelu_erf_grad): cdf + x pdf, pdf = c __expf(a), a = -0.5 x^2.
#   a: 2 U32 |a|; __expf multiplies by log2(e) (constant and product: 2 U32 |a log2e|) before v_exp: relative 4 U32 |a| + ULP2; c *: U32
#   cdf: 0.5 e_sum + U32 cdf; x pdf and the sum: 2 U32 |grad| ; dy *: U32
def gelu_grad_ref(dy, x):
    dy64, x64 = dy.double(), x.double()
    erf, e_sum = _erf_parts(x64)
    cdf = 0.5 * (1 + erf)
    pdf = 0.3989422804014327 * torch.exp(-0.5 * x64 * x64)
    grad = cdf + x64 * pdf
    e_pdf = (4 * 0.5 * x64 * x64 + 2) * U32 + ULP2
    e = 0.5 * e_sum + U32 * cdf.abs() + (x64 * pdf).abs() * (e_pdf + U32) + 2 * U32 * (cdf.abs() + (x64 * pdf).abs())
    ref = dy64 * grad
    return ref, dy64.abs() * e + U32 * ref.abs()


# SwiGLU (swiglu_bf16_kernel): bf16(g * mp_sigmoid_fast(g) * u).  ASSERTED: one bf16 ulp of the exact value plus a floor.  The floor:
# 1 + __expf(-g) exceeds 2^126 for g < -126 ln 2 = -87.34, its reciprocal is then subnormal and v_rcp_f32 returns 0 (for g < -88.7
# __expf overflows and rcp(inf) = 0): the kernel gives -0 where the exact |silu(g)| = |g| e^g <= 87.34 * 2^-126 (|g| e^g falls with
# |g| beyond 1).  Times |u|, plus 2^-126 for a product that is itself subnormal.
def swiglu_ref(gv, uv):
    g64, u64 = gv.double(), uv.double()
    ref = g64 * torch.sigmoid(g64) * u64
    floor = 87.34 * 2.0 ** -126 * u64.abs() + 2.0 ** -126
    return ref, bf16_ulp(ref), floor


def swiglu_sweep():
    """gu [3, 2F] bf16: every finite bf16 g in [-100, 100] (zero padded to a multiple of 8) against u = 1, -1.5, 3e4, one per row."""
    pat = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    g = pat[torch.isfinite(pat.float()) & (pat.float().abs() <= 100)]
    F = (g.numel() + 7) // 8 * 8
    gu = torch.zeros(3, 2 * F, dtype=torch.bfloat16)
    gu[:, :g.numel()] = g
    for r, u in enumerate((1.0, -1.5, 3e4)):
        gu[r, F:] = u
    return gu, g.numel()


# RoPE (rope_qk_bf16_kernel, decode_rope_append_kernel): lo' = bf16(a cos - b sin), hi' = bf16(b cos + a sin) in fp32: two products
# and a sum (or a product and an fma): <= 3 U32 (|a cos| + |b sin|), then the store.
def rope_ref(lo, hi, cos, sin):
    """float64 halves [..., half] and tables broadcastable to them -> (lo', hi', bound_lo, bound_hi)."""
    rl, rh = lo * cos - hi * sin, hi * cos + lo * sin
    el, eh = 3 * U32 * ((lo * cos).abs() + (hi * sin).abs()), 3 * U32 * ((hi * cos).abs() + (lo * sin).abs())
    return rl, rh, U_BF16 * (rl.abs() + el) + el, U_BF16 * (rh.abs() + eh) + eh


# cast_to_bf16: the fp32 values around every rounding tie.
def cast_tie_sweep():
    """fp32 [3 * 65280 + specials + 8]: for every finite bf16 pattern p the exact midpoint between p and its successor in magnitude
    (fp32 bits p << 16 | 0x8000) and the fp32 values one ulp to either side; +-0, +-inf, NaNs, fp32 subnormals, the largest finite
    fp32; and eight ties (both parities of p) at the very end, so that a length cut by 0..3 still ends on ties."""
    p = torch.arange(0, 65536, dtype=torch.int64)
    p = p[(p & 0x7F80) != 0x7F80]                                   # finite bf16 patterns, both signs
    mid = (p << 16) | 0x8000
    body = torch.stack([mid - 1, mid, mid + 1], 1).reshape(-1)
    special = torch.tensor([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FC12345, 0xFFFFFFFF,
                            0x7F80FFFF, 0x00000001, 0x80000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x7F7FFFFF, 0xFF7FFFFF], dtype=torch.int64)
    tail = torch.tensor([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x40008000, 0x40018000, 0x00808000, 0x00818000], dtype=torch.int64)
    allb = torch.cat([body, special, tail])
    allb = torch.where(allb >= 2 ** 31, allb - 2 ** 32, allb).to(torch.int32)
    return allb.view(torch.float32)


def assert_bits_nan(name, got, ref):
    """Equal bits, except that a NaN matches any NaN."""
    g, r = got.detach().cpu(), ref.detach().cpu()
    gn, rn = torch.isnan(g.float()), torch.isnan(r.float())
    diff = (bits(g) != bits(r)) & ~(gn & rn)
    n = int(diff.sum())
    first = int(diff.flatten().nonzero()[0]) if n else -1
    msg = f"{name}: {n}/{g.numel()} elements differ (NaN matches NaN)" + (f", first at {first}: got bits {int(bits(g).flatten()[first]) & 0xFFFFFFFF:#x}, "
                                                                          f"expected {int(bits(r).flatten()[first]) & 0xFFFFFFFF:#x}" if n else "")
    print(msg)
    assert n == 0, msg


# Integer-valued operands: |a|, |b| <= 8 and K <= 4096 keep every partial sum of products below 64 * 4096 = 2^18 < 2^24, so fp32
# sums are exact in any order (sgemm, colsum, the atomic split-K) and must equal float64 bit for bit.
def int_values(shape, seed, lim=8):
    return torch.randint(-lim, lim + 1, shape, generator=gen(seed)).float()


SGEMM_MN = (1, 63, 64, 65, 129)
SGEMM_K = (1, 15, 16, 17, 63, 64, 65, 130)


def sgemm_cases():
    """[(form, M, N, K)]: per operand form every K once, every M and every N at least once (not the cross product), plus the K = 63 / 64
    pair at one ragged (M, N): the 16-deep kernel runs below k_unit = 64, the 64-deep one from there."""
    out = []
    for f, form in enumerate(("NN", "NT", "TN")):
        for i, K in enumerate(SGEMM_K):
            out.append((form, SGEMM_MN[(i + f) % 5], SGEMM_MN[(2 * i + f + 1) % 5], K))
        out += [(form, 65, 65, 63), (form, 65, 65, 64)]
    return out


def sgemm_operands(form, M, N, K, seed, batch=()):
    """Integer-valued (a, b) as STORED for the form, and the float64 product."""
    a, b = int_values(batch + (M, K), seed), int_values(batch + (K, N), seed + 1)
    ref = a.double() @ b.double() + 0.0          # + 0.0: a K = 1 product 0 * -3 is -0 in the library's float64 GEMM; the kernel's fma chain starts at +0
    if form == "NT":
        b = b.transpose(-1, -2).contiguous()
    if form == "TN":
        a = a.transpose(-1, -2).contiguous()
    return a, b, ref


COLSUM_ROWS = (0, 1, 15, 16, 17, 48, 49, 63, 64, 65, 113, 777)
COLSUM_COLS = (1, 63, 64, 65, 130)
