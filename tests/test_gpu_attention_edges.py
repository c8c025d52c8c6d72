"""GPU parity of the attention kernels at tile, mask and split edges, PER KEY: forward v2 (variant 0), the two first-generation variants
(1, 2), the log-sum-exp entry, flash-decode and the backward, against float64 softmax attention on the same bf16-rounded inputs.

Random V averages hundreds of keys and hides a dropped one, so next to it the values are one-hot READOUT rows (kernel_parity.readout_values):
the output's columns are then sums of single probabilities.  The bound is per element, |got - ref| <= c (P @ |V|) with c = 2 * 2^-8 + fp32 terms
derived from the kernels' rounding points (kernel_parity.py, beside attn_fwd_c and attn_bwd_ref_and_tols); there is no absolute tolerance
beyond the flush of denormal probabilities.  Every check prints its worst err / bound before it asserts; the measured figures, the wall time
and the mutation table are in profiles/attention_edge_tests.md."""
import functools
import os
import subprocess
import sys

import pytest
import torch

import kernel_parity as kp

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SWEEP = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257)
VARIANTS = (0, 1, 2, "lse")
WORST = {}                      # group -> worst err / bound seen by this process


def _show(*groups):
    for g in groups:
        for k in sorted(WORST):
            if k.startswith(g):
                print(f"WORST {k}: {WORST[k]:.3f}")


# ------------------------------------------------------------------------------------------------------------------ inputs and references
@functools.lru_cache(maxsize=None)
def _qk(B, Sq, Sk, H, D, seed, kind="small"):
    """float32 tensors holding bf16 values.  small: randn * 0.3, a spread softmax in which every key carries visible mass.
    neg: q = +c, k = -c + jitter with D c^2 / sqrt(D) = 100: every scaled score is about -100, the softmax is that of the jitter."""
    g = torch.Generator().manual_seed(seed)
    if kind == "neg":
        c = (100.0 / D ** 0.5) ** 0.5
        return kp.bf(torch.full((B, Sq, H, D), c)), kp.bf(-c + 0.3 * torch.randn(B, Sk, H, D, generator=g))
    return kp.bf(torch.randn(B, Sq, H, D, generator=g) * 0.3), kp.bf(torch.randn(B, Sk, H, D, generator=g) * 0.3)


@functools.lru_cache(maxsize=None)
def _values(B, Sk, H, D):
    g = torch.Generator().manual_seed(7 + Sk + D)
    out = {"mod": kp.readout_values(Sk, D, "mod")[None, :, None, :].expand(B, Sk, H, D).contiguous()}
    if Sk > D:
        out["div"] = kp.readout_values(Sk, D, "div")[None, :, None, :].expand(B, Sk, H, D).contiguous()
    out["randn"] = kp.bf(torch.randn(B, Sk, H, D, generator=g))
    return out


@functools.lru_cache(maxsize=None)
def _mask(name, B, S):
    """key_valid [B, S] bool by name; batch 1 always differs from batch 0, so a wrong row of the mask shows."""
    if name is None:
        return None
    kv = torch.ones(B, S, dtype=torch.bool)
    kind = name[0]
    if kind == "prefix":
        kv[0, name[1]:] = False
        if B > 1:
            kv[1, S - 3:] = False
    elif kind == "holes":                                   # random holes, key 0 valid
        g = torch.Generator().manual_seed(name[1] + S)
        kv = torch.rand(B, S, generator=g) < 0.7
        kv[:, 0] = True
    elif kind == "tile1":                                   # one whole interior tile invalid
        kv[:, 64:128] = False
        if B > 1:
            kv[1, 130] = False
    elif kind == "first64":                                 # the first tile invalid: the running max is still -inf after it
        kv[:, :64] = False
        if B > 1:
            kv[1, 64] = False
    elif kind == "first70":                                 # under the causal mask queries 0..69 have no admissible key
        kv[:, :70] = False
        if B > 1:
            kv[1, 70:75] = False
    else:
        raise KeyError(name)
    return kv


def _mask_cases(S):
    """(causal, mask name) of section 3 of the issue."""
    out = []
    for causal in (False, True):
        out += [(causal, ("prefix", L)) for L in (1, 63, 64, 65, S - 1)]
        out += [(causal, ("holes", 5)), (causal, ("tile1",))]
    return out + [(False, ("first64",)), (True, ("first70",))]


@functools.lru_cache(maxsize=None)
def _ref(B, Sq, Sk, H, D, causal, mask, seed, kind="small"):
    q, k = _qk(B, Sq, Sk, H, D, seed, kind)
    kv = _mask(mask, B, Sk)
    scale = D ** -0.5
    allowed = kp.attn_allowed(B, Sq, Sk, causal, kv)
    P, lse2 = kp.attn_probs64(q.double(), k.double(), allowed, scale)
    return {"q": q, "k": k, "kv": kv, "P": P, "lse2": lse2, "A": kp.attn_score_mag(q, k, scale), "dead": P.sum(-1) == 0, "allowed": allowed}


def _dev(t, dev):
    return t.to(torch.bfloat16).to(dev)


def _run_fwd(variant, qd, kd, vd, causal, kvd, out=None, sk_dev=None):
    from medplib_amd import ops
    if variant == "lse":
        return ops.attention_fwd_lse(qd, kd, vd, causal=causal, key_valid=kvd, out=out)
    return ops.attention(qd, kd, vd, causal=causal, key_valid=kvd, variant=variant, out=out, sk_dev=sk_dev), None


def _check_out(tag, group, out, r, v, c):
    """One output against P @ V in float64 within c (P @ |V|); rows with no admissible key must be exactly zero."""
    B, Sq, H, D = r["q"].shape
    Sk = r["k"].shape[1]
    v64 = v.double()
    ref = torch.einsum("bhqk,bkhd->bqhd", r["P"], v64)
    bound = c * torch.einsum("bhqk,bkhd->bqhd", r["P"], v64.abs()) + kp.attn_fwd_floor(Sk, float(v64.abs().max()))
    got = out.detach().float().cpu().reshape(B, Sq, H, D)
    kp.ratio_check(tag, got, ref, bound, WORST, group)
    dead = r["dead"].permute(0, 2, 1)                                  # [B, Sq, H]
    if bool(dead.any()):
        assert bool((got[dead] == 0).all()), f"{tag}: a row with no admissible key is not exactly zero"


def _check_lse(tag, group, lse2, r, D):
    B, Sq, H, _ = r["q"].shape
    Sk = r["k"].shape[1]
    got = lse2.detach().double().cpu().reshape(B, H, Sq)
    ref, dead = r["lse2"], r["dead"]
    if bool(dead.any()):
        assert bool((got[dead] == float("inf")).all()), f"{tag}: lse2 of a row with no admissible key is not +inf"
    assert bool(torch.isfinite(got[~dead]).all()), f"{tag}: lse2 is not finite on a row that has keys"
    z = torch.zeros_like(ref)
    refz, gotz = torch.where(dead, z, ref), torch.where(dead, z, got)
    kp.ratio_check(tag + " lse2", gotz, refz, kp.attn_lse2_tol(D, Sk, r["A"], refz.abs()) + z, WORST, group + " lse2")


def _fwd_case(dev, variant, D, Sq, Sk, causal, mask, group, B=2, H=3, kind="small", seed=None):
    r = _ref(B, Sq, Sk, H, D, causal, mask, seed if seed is not None else 1000 + Sq + 3 * Sk + D, kind)
    c = kp.attn_fwd_c(D, Sk, r["A"])
    qd, kd = _dev(r["q"], dev), _dev(r["k"], dev)
    kvd = None if r["kv"] is None else r["kv"].to(torch.uint8).to(dev)
    tag = f"v{variant} D={D} Sq={Sq} Sk={Sk} causal={int(causal)} mask={mask} {kind}"
    for name, v in _values(B, Sk, H, D).items():
        out, lse2 = _run_fwd(variant, qd, kd, _dev(v, dev), causal, kvd)
        _check_out(f"{tag} V={name}", group, out, r, v, c)
        if lse2 is not None and name == "randn":
            _check_lse(tag, group, lse2, r, D)
    return r


def run_length_sweep(dev, variant, D):
    for causal in (False, True):
        for S in SWEEP:
            _fwd_case(dev, variant, D, S, S, causal, None, "fwd sweep")


def run_mask_cases(dev, variant, D):
    for S in (200, 257):
        for causal, mask in _mask_cases(S):
            _fwd_case(dev, variant, D, S, S, causal, mask, "fwd masks")


# ------------------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("variant", VARIANTS)
def test_forward_length_sweep(dev, variant, D):
    """Sq = Sk over every tile edge (16, 32, 64, 128, 192, 256 and one to either side), causal and not.  For the lse entry also lse2
    against float64 logsumexp * log2(e) within the derived fp32 bound (kernel_parity.attn_lse2_tol)."""
    run_length_sweep(dev, variant, D)
    _show("fwd sweep")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("variant", VARIANTS)
def test_forward_masks_with_holes_and_dead_rows(dev, variant, D):
    """key_valid is read per key: prefixes of 1, 63, 64, 65 and S - 1 keys, random holes, a whole interior tile invalid, the first tile invalid
    (the m_safe path: the running max is -inf after a whole tile) and, under the causal mask, keys 0..69 invalid, which leaves queries 0..69
    without any admissible key.  Pinned for such rows: the output is exactly 0 and lse2 is +inf, every other row is finite."""
    run_mask_cases(dev, variant, D)
    _show("fwd masks")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("variant", VARIANTS)
def test_forward_sq_differs_from_sk(dev, variant, D):
    """The tiled kernels with Sq != Sk (top-left aligned causal mask): the `causal && Sq <= Sk` shortcut of v2 and its Sq > Sk sibling,
    and one query against 200 masked keys (the mask keeps it off the decode path)."""
    for causal in (False, True):
        for Sq, Sk in ((5, 200), (200, 70), (130, 129), (64, 65)):
            _fwd_case(dev, variant, D, Sq, Sk, causal, None, "fwd Sq!=Sk")
        _fwd_case(dev, variant, D, 1, 200, causal, ("holes", 9), "fwd Sq!=Sk")
    _show("fwd Sq!=Sk")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_forward_sk_dev_on_the_tiled_kernels(dev, variant, D):
    """A device-side key count on the tiled path (Sq > 1): the result is attention over the truncated K / V.  All three variants honour
    sk_dev (the lse entry takes none).  With a key_valid mask the mask's rows keep the TENSOR's length: batch 1 must read its own row."""
    B, H, Sq, Sk = 2, 3, 130, 300
    for causal in (False, True):
        for mask in (None, ("holes", 3)):
            q, k = _qk(B, Sq, Sk, H, D, 4000 + D)
            kv = _mask(mask, B, Sk)
            qd, kd = _dev(q, dev), _dev(k, dev)
            kvd = None if kv is None else kv.to(torch.uint8).to(dev)
            vals = {n: (v, _dev(v, dev)) for n, v in _values(B, Sk, H, D).items()}
            for n in (1, 64, 65, 299):
                allowed = kp.attn_allowed(B, Sq, n, causal, None if kv is None else kv[:, :n])
                P, lse2 = kp.attn_probs64(q.double(), k[:, :n].double(), allowed, D ** -0.5)
                r = {"q": q, "k": k[:, :n], "P": P, "dead": P.sum(-1) == 0}
                c = kp.attn_fwd_c(D, n, kp.attn_score_mag(q, k[:, :n], D ** -0.5))
                nd = torch.tensor([n], dtype=torch.int32, device=dev)
                for name, (v, vd) in vals.items():
                    out, _ = _run_fwd(variant, qd, kd, vd, causal, kvd, sk_dev=nd)
                    _check_out(f"v{variant} D={D} sk_dev={n}/{Sk} causal={int(causal)} mask={mask} V={name}", "fwd sk_dev", out, r, v[:, :n], c)
    _show("fwd sk_dev")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("variant", VARIANTS)
def test_forward_strided_output_keeps_the_padding(dev, variant, D):
    """An out= view with a wider row stride (H * D + 64, what training passes): the columns past H * D keep their bits."""
    B, H, S = 2, 3, 130
    r = _ref(B, S, S, H, D, True, None, 5000 + D)
    v = _values(B, S, H, D)["randn"]
    buf = torch.full((B, S, H * D + 64), -7.25, dtype=torch.bfloat16, device=dev)
    before = kp.bits(buf[:, :, H * D:])
    out, _ = _run_fwd(variant, _dev(r["q"], dev), _dev(r["k"], dev), _dev(v, dev), True, None, out=buf[:, :, :H * D])
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr()
    _check_out(f"v{variant} D={D} strided out", "fwd strided", out, r, v, kp.attn_fwd_c(D, S, r["A"]))
    assert torch.equal(kp.bits(buf[:, :, H * D:]), before), "the kernel wrote past H * D columns of a strided output row"


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("variant", VARIANTS)
def test_forward_all_scores_very_negative(dev, variant, D):
    """Every scaled score about -100: the shift by the row max from the other side than the dominant-key test.  Finite and within the
    bound (whose fp32 score term is no longer negligible: A ~ 100), causal and with ragged masks."""
    for causal, mask in ((True, None), (False, ("prefix", 187)), (True, ("holes", 11))):
        _fwd_case(dev, variant, D, 200, 200, causal, mask, "fwd negative", kind="neg", seed=6000 + D)
    _show("fwd negative")


# ------------------------------------------------------------------------------------------------------------------------------- decode
DEC_SWEEP = (1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 2047, 2048, 2049, 2065, 4095, 8191)


def _decode_splits(BH, Sk):
    """The split count launch_attn_decode chooses with the workspace registered (restated: it only selects the merge term of the bound)."""
    ns = min(16, 256 // BH) if BH <= 256 else 1
    while (Sk + ns - 1) // ns + 64 > 2048:
        ns += 1
    return ns


def _decode_lengths(dev, B, H, D, lengths, cache_len, group, modes=("sk_dev", "tensor")):
    from medplib_amd import ops
    q, k = _qk(B, 1, cache_len, H, D, 7000 + B * H + D)
    vals = _values(B, cache_len, H, D)
    qd, kd = _dev(q, dev), _dev(k, dev)
    vds = {n: _dev(v, dev) for n, v in vals.items()}
    for Sk in lengths:
        P, _ = kp.attn_probs64(q.double(), k[:, :Sk].double(), torch.ones(B, 1, 1, Sk, dtype=torch.bool), D ** -0.5)
        r = {"q": q, "k": k[:, :Sk], "P": P, "dead": P.sum(-1) == 0}
        A = kp.attn_score_mag(q, k[:, :Sk], D ** -0.5)
        kt = kd[:, :Sk].contiguous()
        for name, v in vals.items():
            vt = vds[name][:, :Sk].contiguous()
            tiled = ops.attention(qd, kt, vt, causal=False, variant=2)
            for mode in modes:
                if mode == "sk_dev":
                    args, kw, host_len = (qd, kd, vds[name]), {"sk_dev": torch.tensor([Sk], dtype=torch.int32, device=dev)}, cache_len
                else:
                    args, kw, host_len = (qd, kt, vt), {}, Sk
                c = kp.attn_fwd_c(D, Sk, A, splits=_decode_splits(B * H, host_len) if host_len <= 31744 else 0)   # longer: the tiled kernel
                out = ops.attention(*args, causal=False, **kw)
                again = ops.attention(*args, causal=False, **kw)
                tag = f"decode D={D} BH={B * H} Sk={Sk} ({mode}) V={name}"
                _check_out(tag, group, out, r, v[:, :Sk], c)
                assert torch.equal(kp.bits(out), kp.bits(again)), f"{tag}: the second call differs (arrival tickets not reset?)"
                # decode against the tiled kernel: each is within its own bound of the same reference (triangle inequality), so the two
                # differ by at most the sum of their bounds
                v64 = v[:, :Sk].double()
                both = (c + kp.attn_fwd_c(D, Sk, A)) * torch.einsum("bhqk,bkhd->bqhd", P, v64.abs()) + 2 * kp.attn_fwd_floor(Sk, float(v64.abs().max()))
                kp.ratio_check(tag + " vs tiled", out.float().cpu().reshape(B, 1, H, D), tiled.double().cpu().reshape(B, 1, H, D), both, WORST, group + " vs tiled")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("B,H", [(2, 4), (1, 1)])
def test_decode_length_sweep(dev, B, H, D):
    """Sq = 1 with 16 splits: lengths around the chunk rounding (16 / 32 keys), around the short-split limit (128 / 256 keys per split) and
    into the general loop, as a device-side count on a longer cache and as the tensor's own length; every call twice (equal bits)."""
    _decode_lengths(dev, B, H, D, DEC_SWEEP, 8200, "decode sweep")
    _show("decode sweep")
    _qk.cache_clear(); _values.cache_clear()


@pytest.mark.parametrize("D", [64, 128])
def test_decode_fewer_splits(dev, D):
    """B * H = 64 -> 4 splits; B * H = 300 -> one split (no workspace use, the kernel normalises itself)."""
    _decode_lengths(dev, 2, 32, D, (257, 1025), 1030, "decode NS=4")
    _decode_lengths(dev, 2, 150, D, (129,), 140, "decode NS=1")
    if D == 64:                                  # (the long one at one head size: 300 heads x 1984 keys is the module's largest tensor)
        _decode_lengths(dev, 2, 150, D, (1984,), 1984, "decode NS=1", modes=("tensor",))
    _show("decode NS")
    _qk.cache_clear(); _values.cache_clear()


@pytest.mark.parametrize("D", [64, 128])
def test_decode_split_limit(dev, D):
    """One head, one query: 31744 keys = 16 splits of 1984 (the most a split's LDS score array takes), and 31745 keys, which falls through
    to the tiled kernel."""
    _decode_lengths(dev, 1, 1, D, (31744, 31745), 31745, "decode limit", modes=("tensor",))
    _show("decode limit")
    _qk.cache_clear(); _values.cache_clear()


# ----------------------------------------------------------------------------------------------------------------------------- backward
BWD_SWEEP = (1, 17, 63, 64, 65, 127, 128, 129, 193, 257)


def _bwd_case(dev, D, S, causal, mask, group, B=2, H=2):
    from medplib_amd import ops
    r = _ref(B, S, S, H, D, causal, mask, 8000 + S + D)
    g = torch.Generator().manual_seed(8100 + S + D)
    v = kp.bf(torch.randn(B, S, H, D, generator=g))
    d_outs = {"randn": kp.bf(torch.randn(B, S, H * D, generator=g)),
              "readout": kp.readout_values(S, D, "mod")[None, :, None, :].expand(B, S, H, D).reshape(B, S, H * D).contiguous()}
    qd, kd, vd = _dev(r["q"], dev), _dev(r["k"], dev), _dev(v, dev)
    kvd = None if r["kv"] is None else r["kv"].to(torch.uint8).to(dev)
    c_fwd = kp.attn_fwd_c(D, S, r["A"])
    lse_tol = float(kp.attn_lse2_tol(D, S, r["A"], float(r["lse2"][~r["dead"]].abs().max())))
    out, lse2 = ops.attention_fwd_lse(qd, kd, vd, causal=causal, key_valid=kvd)
    tag0 = f"bwd D={D} S={S} causal={int(causal)} mask={mask}"
    _check_out(tag0 + " (its forward)", group + " fwd", out, r, v, c_fwd)
    for gname, d_out in d_outs.items():
        t = kp.attn_bwd_ref_and_tols(r["q"], r["k"], v, d_out, r["allowed"], D ** -0.5, c_fwd, lse_tol, r["A"])
        for fused in (True, False):             # mp_attention_bwd_fused_bf16 / mp_attention_delta_bf16 + mp_attention_bwd_bf16
            dq, dk, dv, _ = ops.attention_bwd(qd, kd, vd, out, _dev(d_out, dev), lse2, causal=causal, key_valid=kvd, fused_delta=fused)
            torch.cuda.synchronize()
            for n, got in (("dq", dq), ("dk", dk), ("dv", dv)):
                kp.ratio_check(f"{tag0} dO={gname} fused={int(fused)} {n}", got.float().cpu(), t[n], t["tol_" + n], WORST, f"{group} {n}")
            if r["kv"] is not None:             # an invalid key receives exactly no gradient, wherever it sits
                inv = ~r["kv"]
                assert bool((dk.float().cpu()[inv] == 0).all()) and bool((dv.float().cpu()[inv] == 0).all()), tag0 + ": gradient at an invalid key"
            dead = r["dead"].permute(0, 2, 1)   # [B, S, H]: a query without keys gets exactly zero dQ
            if bool(dead.any()):
                assert bool((dq.float().cpu()[dead] == 0).all()), tag0 + ": dQ of a row with no admissible key"


@pytest.mark.parametrize("D", [64, 128])
def test_backward_length_sweep(dev, D):
    """Both backward entry points against float64 autograd, causal, per element within the bounds written beside
    kernel_parity.attn_bwd_ref_and_tols; dO random and as a readout (dO[q] = e_{q mod D}: dV's columns are marginals of P^T)."""
    for S in BWD_SWEEP:
        _bwd_case(dev, D, S, True, None, "bwd sweep")
    _show("bwd sweep")


@pytest.mark.parametrize("D", [64, 128])
def test_backward_masks(dev, D):
    """The masks of the forward cases at S = 200: zero gradient at every invalid key (holes included), zero dQ on rows without keys."""
    for causal, mask in _mask_cases(200):
        if causal or mask == ("first64",):
            _bwd_case(dev, D, 200, causal, mask, "bwd masks")
    _show("bwd masks")


@pytest.mark.parametrize("D", [64, 128])
def test_backward_non_causal(dev, D):
    """causal = 0 is accepted by both backward entry points: the same bounds."""
    for S in (65, 129, 200):
        _bwd_case(dev, D, S, False, None, "bwd non-causal")
    _bwd_case(dev, D, 200, False, ("holes", 5), "bwd non-causal")
    _show("bwd non-causal")


# ---------------------------------------------------------------------------------------------------------------------------- A/B forms
def test_ab_forms_of_the_v2_kernel(dev):
    """MP_ATTN_KT=32, MP_ATTN_TUNED=0 and MP_ATTN_PLAIN=0 are read once per process: one fresh child each, one after another, running the
    length sweep and the mask cases for variant 0 with the same bounds (tests/_attn_edges_worker.py).  Stops at the first child that fails."""
    for setting in ("MP_ATTN_KT=32", "MP_ATTN_TUNED=0", "MP_ATTN_PLAIN=0"):
        name, value = setting.split("=")
        env = {k: v for k, v in os.environ.items() if not k.startswith("MP_ATTN_")}
        env[name] = value
        try:
            p = subprocess.run([sys.executable, os.path.join(HERE, "_attn_edges_worker.py")], env=env, capture_output=True, text=True, timeout=120)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"{setting}: the child did not finish in 120 s\n{str(e.stdout)[-3000:]}\n{str(e.stderr)[-3000:]}")
        print(setting, "rc", p.returncode, "\n".join(line for line in p.stdout.splitlines() if line.startswith("WORST")))
        assert p.returncode == 0, f"{setting}: the child failed\n{p.stdout[-4000:]}\n{p.stderr[-4000:]}"
        assert "attn-edges-worker ok" in p.stdout, f"{setting}: the child ended without its last line\n{p.stdout[-2000:]}"
