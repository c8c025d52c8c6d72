"""Helper of tests/test_gpu_gemv_edges.py (not collected): exact operands, float64 references, the dispatch of the decode GEMV entry points
restated in Python, and the case table.  tests/test_gemv_cases.py checks all of it on the CPU.

Operands.  "Grid" weights W = c * 2^e (c an integer in [-127, 127] with one +-127 per row, e per row in [-12, -5]) are exact in bf16 and
are their own int8 codes with scale 2^e; activations are integers in [-4, 4].  Every partial sum of x . W[n] is then an integer below
127 * 4 * K < 2^24 times 2^e: exact in fp32 in ANY association, so every kernel that computes the dot product must return the same fp32
number.  The epilogue operands keep the later steps exact up to the roundings the kernels document (gemv_epilogue.h): alpha in {1, 0.5},
bias an integer times the row's 2^e, combine weights with three mantissa bits (times a bf16's eight: exact in fp32, so fma and mul + add
agree), activation NONE or ReLU.  The references below are float64 with those roundings written out, each `.float()` one fp32 rounding of
an exact float64 value."""
import functools
from collections import namedtuple
from types import SimpleNamespace

import torch

ACT_NONE, ACT_RELU, ACT_SWIGLU_PAIR = 0, 1, 5
SCALES = (0.5, 0.75, 1.0, 1.25)
E = 3                                                          # experts of every indexed case; expert 1 is never selected


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ operands
def grid(g, *shape):
    """Grid weights [..., N, K] -> (w bf16, c int16 [..., N, K], e int64 [..., N])."""
    c = torch.randint(-127, 128, shape, generator=g, dtype=torch.int16)
    at = torch.randint(0, shape[-1], shape[:-1] + (1,), generator=g)
    sign = (torch.randint(0, 2, shape[:-1] + (1,), generator=g) * 2 - 1).to(torch.int16)
    c.scatter_(-1, at, 127 * sign)
    e = torch.randint(-12, -4, shape[:-1], generator=g)
    exact = c.float() * torch.pow(torch.tensor(2.0), e.float()).unsqueeze(-1)
    w = exact.to(torch.bfloat16)
    assert torch.equal(w.float(), exact)
    return w, c, e


def ints(g, M, K):
    return torch.randint(-4, 5, (M, K), generator=g).float().to(torch.bfloat16)


def eighths(g, M, N):
    """A residual: multiples of 1/8 in [-8, 8] (exact in bf16), so residual + anything above is an exact float64 sum."""
    return (torch.randint(-64, 65, (M, N), generator=g).float() / 8).to(torch.bfloat16)


def bias_on(g, e):
    """fp32 bias [N]: an integer |.| <= 1000 times row n's 2^e."""
    return torch.randint(-1000, 1001, e.shape, generator=g).float() * torch.pow(torch.tensor(2.0), e.float())


def weights3(g, n):
    return torch.tensor(SCALES)[torch.randint(0, len(SCALES), (n,), generator=g)]


def pow2(e):
    return torch.pow(torch.tensor(2.0), e.float())


# ------------------------------------------------------------------------------------------------ float64 references
def bf(v64):
    """float64 -> fp32 -> bf16, the kernels' (bf16_t)(float) of a value that was computed in fp32."""
    return v64.float().to(torch.bfloat16)


def is_f32(v64):
    return torch.equal(v64.float().double(), v64)


def dot64(x, w):
    """x [M, K] . w [N, K] -> [M, N] float64 (+0 where the sum cancels, as an fp32 chain that starts from +0 gives)."""
    return x.double() @ w.double().T + 0.0


def dot64_indexed(x, w, idx):
    """Row m against expert idx[m] of w [E, N, K]."""
    return torch.stack([dot64(x[m:m + 1], w[idx[m]])[0] for m in range(x.shape[0])])


def ref_shared(a, alpha=1.0, bias=None, act=ACT_NONE, residual=None, out_f32=False):
    """gv_store_shared: act(a * alpha + bias) -> bf16 rounding unless fp32 output -> + residual -> output rounding."""
    v = a * alpha + (bias.double() if bias is not None else 0.0)
    if act == ACT_RELU:
        v = v.clamp_min(0.0)
    if out_f32:
        return (v + residual.double()).float() if residual is not None else v.float()
    v = bf(v)
    return bf(v.double() + residual.double()) if residual is not None else v


def ref_indexed(a, scale=None, residual=None, keep=None):
    """gv_store_indexed per row: bf16(scale * bf16(a) + residual); a capacity-dropped row is the residual's own bits, +0 without one."""
    rows = []
    for m in range(a.shape[0]):
        if keep is not None and keep[m] < 0:
            rows.append(residual[m] if residual is not None else torch.zeros(a.shape[1], dtype=torch.bfloat16))
            continue
        v = (float(scale[m]) if scale is not None else 1.0) * bf(a[m]).double()
        rows.append(bf(v.float().double() + residual[m].double()) if residual is not None else bf(v))
    return torch.stack(rows)


def ref_top2_down(dots, weight, keep, residual):
    """gemv_top2_down_kernel: acc = fma(w_c, bf16(dot_c), acc) over the kept choices c = 0, 1 of token t (entry c * T + t), then
    bf16(residual + acc); dots [2T, N] float64."""
    T = dots.shape[0] // 2
    acc = torch.zeros(T, dots.shape[1], dtype=torch.float64)
    for c in range(2):
        for t in range(T):
            if keep[c * T + t] >= 0:
                acc[t] = (float(weight[c * T + t]) * bf(dots[c * T + t]).double() + acc[t]).float().double()
    return bf(residual.double() + acc) if residual is not None else bf(acc)


def swiglu_halves(w):
    """Interleaved gate|up rows [..., N, K] (blocks of 32 gate rows, then their 32 up rows) -> (gate, up) [..., N / 2, K]."""
    v = w.reshape(w.shape[:-2] + (w.shape[-2] // 64, 2, 32, w.shape[-1]))
    half = w.shape[:-2] + (w.shape[-2] // 2, w.shape[-1])
    return v[..., 0, :, :].reshape(half), v[..., 1, :, :].reshape(half)


# ------------------------------------------------------------------------------------------------ the dispatch, restated
def ksplit_terms(M, N, K, indexed):
    """The three terms of the K-split predicate of mp_gemv_bf16 / mp_gemv_w8_bf16."""
    return (N <= 4096, K >= 4096, bool(indexed) or M == 1)


def route(M, N, K, indexed, swiglu, w8):
    """-> (kernel, passes): which kernel mp_gemv_bf16 (w8 False) or mp_gemv_w8_bf16 (w8 True) launches, "ksplit" | "indexed" | "shared", and
    for "shared" the rows of each pass — (M,) up to four rows, (4, M - 4) above.  Both entry points carry the same predicate (the bf16 one
    with its default MP_GEMV_KSPLIT); `w8` is an argument so that a change to either shows here."""
    assert 1 <= M <= 8
    if not swiglu and all(ksplit_terms(M, N, K, indexed)):
        return "ksplit", None
    if indexed:
        return "indexed", None
    return "shared", ((M,) if M <= 4 else (4, M - 4))


# ------------------------------------------------------------------------------------------------ the case table
Case = namedtuple("Case", "w8 indexed M N K seed")

N_ALL = (1, 2, 3, 5, 17, 66, 130)
N_SWIGLU = (64, 128, 192)
N_KSPLIT = (3, 17, 66)
K_SHARED = {False: (8, 504, 512, 520, 1024, 1536, 1544), True: (16, 1008, 1024, 1040, 2048, 3088)}
K_INDEXED = {False: (8, 520, 2048, 2056, 2560), True: (16, 1040, 2048, 3088)}
K_KSPLIT = {False: (4096, 4104, 4608, 6144, 6152, 8192), True: (4096, 4112, 5120, 8192, 8208)}
M_INDEXED = (1, 4, 8)
TOKENS = (1, 3, 8)

# (M, N, K) per form; w8 False / True.  Every N, K and M of the lists above at least once per form, ragged N with ragged K at least once.
_SHARED = {False: ((1, 1, 8), (2, 2, 504), (3, 3, 512), (4, 5, 520), (5, 17, 1024), (6, 66, 1536), (7, 130, 1544), (8, 3, 1544), (5, 2, 8)),
           True: ((1, 1, 16), (2, 2, 1008), (3, 3, 1024), (4, 5, 1040), (5, 17, 2048), (6, 66, 3088), (7, 130, 1040), (8, 3, 3088), (5, 2, 16))}
_INDEXED = {False: ((1, 1, 8), (4, 2, 520), (8, 3, 2048), (1, 5, 2056), (4, 17, 2560), (8, 66, 520), (4, 130, 2056)),
            True: ((1, 1, 16), (4, 2, 1040), (8, 3, 2048), (1, 5, 3088), (4, 17, 1040), (8, 66, 3088), (4, 130, 16))}
_KSPLIT = {False: ((1, 3, 4096), (1, 17, 4104), (1, 66, 4608), (1, 3, 6144), (1, 17, 6152), (1, 66, 8192)),
           True: ((1, 3, 4096), (1, 17, 4112), (1, 66, 5120), (1, 3, 8192), (1, 17, 8208), (1, 66, 4112))}
_KSPLIT_INDEXED = {False: ((4, 3, 4096), (8, 17, 4104), (1, 66, 4608), (4, 66, 6144), (8, 3, 6152), (1, 17, 8192)),
                   True: ((4, 3, 4096), (8, 17, 4112), (1, 66, 5120), (4, 66, 8192), (8, 3, 8208), (1, 17, 4112))}


def _cases(table, w8, indexed, seed0):
    return [Case(w8, indexed, M, N, K, seed0 + i) for i, (M, N, K) in enumerate(table[w8])]


def shared_cases(w8):
    """One matrix for all rows: the wave-per-four-rows kernel (M = 1..8) and, at M = 1 with a long K, the K-split kernel."""
    return _cases(_SHARED, w8, False, 100) + _cases(_KSPLIT, w8, False, 200)


def indexed_cases(w8):
    """A matrix per row (E = 3): the wave-per-four-rows indexed kernel and the K-split kernel."""
    return _cases(_INDEXED, w8, True, 300) + _cases(_KSPLIT_INDEXED, w8, True, 400)


def both_types_cases():
    """Every case of either table whose K both entry points accept (K % 16 == 0), as bf16 cases: the int8 entry runs them too."""
    seen, out = set(), []
    for w8 in (False, True):
        for c in shared_cases(w8) + indexed_cases(w8):
            key = (c.indexed, c.M, c.N, c.K)
            if c.K % 16 == 0 and key not in seen:
                seen.add(key)
                out.append(c._replace(w8=False))
    return out


# SwiGLU pairing (N % 64 == 0), K a multiple of 16 so that both weight types run every case
SWIGLU_SHARED = ((1, 64, 16), (2, 128, 1040), (3, 192, 2048), (4, 64, 1040), (5, 128, 16), (6, 192, 1040), (7, 64, 2048), (8, 128, 1040))
SWIGLU_INDEXED = ((1, 64, 16), (3, 128, 1040), (8, 192, 2048), (3, 64, 2560))           # (T, N, K): T tokens, 2T (token, choice) entries
TOP2_DOWN = ((1, 3, 4096), (3, 17, 4104), (8, 66, 4608), (3, 66, 8), (8, 3, 520), (1, 17, 4608))     # (T, N, K)
QUANT_K = (16, 240, 256, 272)
QUANT_ROWS = (1, 3)


def expert_of_rows(M):
    """w_index of an indexed case: experts 2 and 0 in turn.  Expert 1 (and at M = 1 expert 0) is selected by no row: its matrix is poison."""
    return [(2, 0)[m % 2] for m in range(M)]


@functools.lru_cache(maxsize=None)
def operands(case):
    """The operands of a case on the CPU, from its seed alone: x, w (c, e), a residual, a bias, and for an indexed case idx / row_scale.
    Built once per case and shared by the tests: nobody writes to them."""
    g = gen(case.seed)
    shape = (E, case.N, case.K) if case.indexed else (case.N, case.K)
    w, c, e = grid(g, *shape)
    o = SimpleNamespace(case=case, M=case.M, N=case.N, K=case.K, w=w, c=c, e=e, x=ints(g, case.M, case.K), res=eighths(g, case.M, case.N),
                        idx=None, row_scale=None, bias=None)
    if case.indexed:
        o.idx, o.row_scale = expert_of_rows(case.M), weights3(g, case.M)
        o.a = dot64_indexed(o.x, w, o.idx)
    else:
        o.bias = bias_on(g, e)
        o.a = dot64(o.x, w)
    return o


def keep_patterns(M):
    """name -> row_keep [M] (a slot number, < 0 = dropped by the capacity limit); patterns that coincide at this M appear once."""
    pats = {"none": list(range(M)), "first": [-1] + list(range(1, M)), "last": list(range(M - 1)) + [-1], "all": [-1] * M}
    out = {}
    for name, p in pats.items():
        if p not in out.values():
            out[name] = p
    return out


TOKEN_KINDS = ("both", "first_only", "second_only", "neither")


def top2_patterns(T):
    """name -> slot [2T] of the entries e = c * T + t: the four patterns of keep_patterns over the entries, and "mixed", where token t keeps
    both, only its first, only its second, neither choice in turn."""
    out = keep_patterns(2 * T)
    mixed = list(range(2 * T))
    for t in range(T):
        if t % 4 in (2, 3):
            mixed[t] = -1
        if t % 4 in (1, 3):
            mixed[T + t] = -1
    if mixed not in out.values():
        out["mixed"] = mixed
    return out


def token_kinds(slot):
    T = len(slot) // 2
    return {TOKEN_KINDS[(slot[t] < 0) * 2 + (slot[T + t] < 0)] for t in range(T)}


def top2_experts(T):
    """expert [2T]: first choices 2, 0, 2, ...; second choices 0, 2, 0, ...; expert 1 is poison."""
    return [(2, 0)[t % 2] for t in range(T)] + [(0, 2)[t % 2] for t in range(T)]


@functools.lru_cache(maxsize=None)
def top2_operands(T, N, K, seed, swiglu):
    """gate|up (swiglu): x [T, K]; down: act [2T, K].  w [E, N, K] grid, residual [T, N], combine weights [2T]."""
    g = gen(seed)
    w, c, e = grid(g, E, N, K)
    return SimpleNamespace(T=T, N=N, K=K, w=w, c=c, e=e, x=ints(g, T if swiglu else 2 * T, K), res=eighths(g, T, N), expert=top2_experts(T),
                           weight=weights3(g, 2 * T))


# ------------------------------------------------------------------------------------------------ the K-split predicate, crossed
def _plain(w8, M, N, K, w, c, e, x, res):
    return SimpleNamespace(case=Case(w8, False, M, N, K, 0), M=M, N=N, K=K, w=w, c=c, e=e, x=x, res=res, idx=None, row_scale=None, bias=None,
                           a=dot64(x, w))


@functools.lru_cache(maxsize=None)
def predicate_pairs(w8):
    """[(term, left, right, rows, cols)]: two plain launches that differ in ONE term of `N <= 4096 && K >= 4096 && (w_index || M == 1)` and
    compute the same sums on y[:rows, :cols] — the left one takes the K-split kernel, the right one the wave-per-four-rows kernel.
      N: 4096 against 4100 rows of the same matrix.   K: 4096 against 4088 (int8: 4080) columns, the rest of W and x zero.
      M: one row against two, row 0 the same."""
    out = []
    g = gen(500)
    w, c, e = grid(g, 4100, 4096)
    x, res = ints(g, 1, 4096), eighths(g, 1, 4100)
    out.append(("N", _plain(w8, 1, 4096, 4096, w[:4096], c[:4096], e[:4096], x, res[:, :4096]), _plain(w8, 1, 4100, 4096, w, c, e, x, res), 1, 4096))
    g = gen(510)
    short = 4080 if w8 else 4088
    ws, cs, e = grid(g, 64, short)                             # the +-127 of every row lies in the first `short` columns: one absmax
    xs, res = ints(g, 1, short), eighths(g, 1, 64)
    w = torch.zeros(64, 4096, dtype=torch.bfloat16); w[:, :short] = ws
    c = torch.zeros(64, 4096, dtype=torch.int16); c[:, :short] = cs
    x = torch.zeros(1, 4096, dtype=torch.bfloat16); x[:, :short] = xs
    out.append(("K", _plain(w8, 1, 64, 4096, w, c, e, x, res), _plain(w8, 1, 64, short, ws, cs, e, xs, res), 1, 64))
    g = gen(520)
    w, c, e = grid(g, 64, 4096)
    x, res = ints(g, 2, 4096), eighths(g, 2, 64)
    out.append(("M", _plain(w8, 1, 64, 4096, w, c, e, x[:1], res[:1]), _plain(w8, 2, 64, 4096, w, c, e, x, res), 1, 64))
    return out
