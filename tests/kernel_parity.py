"""Helpers shared by the kernel-level parity tests (test_gpu_train_kernels.py, test_gpu_glue_kernels.py, test_gpu_attention_edges.py)
and the crafted MoE routing cases their CPU guard checks (test_kernel_coverage.py).  Plain torch on the CPU only: nothing here touches the GPU."""
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
