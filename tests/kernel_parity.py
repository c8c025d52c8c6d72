"""Helpers shared by the kernel-level parity tests (test_gpu_train_kernels.py, test_gpu_glue_kernels.py) and the crafted MoE
routing cases their CPU guard checks (test_kernel_coverage.py).  Plain torch on the CPU only: nothing here touches the GPU."""
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
