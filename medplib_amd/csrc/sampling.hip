// Sampling of the next token on the device: the temperature pick (the serving worker's softmax(logits / T) + multinomial pick; greedy decoding
// keeps mp_argmax_rows_f32 in norm_elementwise.hip), and top-k / top-p truncation in front of it (HF 4.31's warper chain
// TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> multinomial, what the reference's vqa_infer.py:430-442 asks of
// generate(do_sample=True, temperature=, top_p=)).  gfx950, wave64.
#include "row_pick.h"

namespace {

using namespace row_pick;

// w_j = exp((l_j - max l) / T): a column equal to the maximum has w = 1 exactly (also when the maximum is +inf, where l - max is not a number)
__device__ __forceinline__ float temperature_weight(float l, float m, float inv_t) { return l == m ? 1.f : __expf((l - m) * inv_t); }

// Inverse-CDF pick of one column per row: out = the smallest i with w_i > 0 whose cumulative weight C(i) exceeds u * C(cols - 1).  One block
// per row in the geometry of row_pick.h:
//   1. row maximum (block reduction), weights in place of the logits;
//   2. row_pick::inverse_cdf_pick over them.
// The same row, u and T give the same column on every launch, for every alignment of the row and whatever rows share the launch.  Columns at
// or past `cols` (loaded as -inf) and every column of a row without a maximum above -inf (all -inf, all NaN) weigh 0, whatever they compare
// equal to: such a row gives 0, and columns past `cols` are never picked.  NaN columns beside finite ones weigh nothing and make C NaN, which
// ends at the last column with w > 0.
// (The body is a device function of the block's row r, its draw *u and its token *out: sample_rows_kernel runs it with the launch's one
// temperature, pick_rows_kernel below with the row's own.)
template <int K, bool KEEP>
__device__ __forceinline__ void sample_row(const float* __restrict__ r, int cols, float inv_t, const float* __restrict__ u, int64_t* __restrict__ out) {
  __shared__ float red[16];
  const bool wide = starts_on_16_bytes(r);
  auto piece = [&](int k) { return load_piece(r, wide, cols, -INFINITY, k); };
  float4 v[KEEP ? K : 1];                    // KEEP: the row stays in registers
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float4 p = piece(k);
    if constexpr (KEEP) v[k] = p;
    m = fmaxf(m, piece_max(p));
  }
  m = block_max(m, red);

  const bool has_max = m > -INFINITY;
  auto weight = [&](float l, int i) { return (has_max && i < cols) ? temperature_weight(l, m, inv_t) : 0.f; };
  inverse_cdf_pick<K, KEEP>(
      [&](int k) {
        float4 p = KEEP ? v[KEEP ? k : 0] : piece(k);
        const int i = piece_column(k);
        p.x = weight(p.x, i); p.y = weight(p.y, i + 1); p.z = weight(p.z, i + 2); p.w = weight(p.w, i + 3);
        return p;
      },
      u, cols, out);
}
template <int K, bool KEEP>
__global__ __launch_bounds__(1024) void sample_rows_kernel(const float* __restrict__ x, int64_t ld, int cols, float inv_t,
                                                           const float* __restrict__ u, int64_t* __restrict__ out) {
  sample_row<K, KEEP>(x + (int64_t)blockIdx.x * ld, cols, inv_t, u + blockIdx.x, out + blockIdx.x);
}

// The truncated pick, in the same geometry.  The truncation is a threshold on the logit, `cut`: a column is kept iff l >= cut.
//   1. row maximum m; a row without one above -inf (all -inf, all NaN) keeps nothing: token 0, kept 0, cut +inf.
//   2. top-k: t_k = the k-th largest logit counting multiplicity, found by bisection on the order-preserving integer key of a float
//      over [key(-inf), key(m)]: every round counts the columns with l >= candidate over the block.  The count
//      is an integer and the compare is on the logits themselves, so the selection is exact and ties at t_k all survive.  The descent
//      stops early at a candidate that exactly k columns reach; t_k is then the smallest of those.  NaN columns (and the padding past
//      `cols`, loaded as NaN) compare false and never count.  Without top-k, t_k = the smallest non-NaN logit.
//   3. top-p over the survivors {l >= t_k}: with w the weights of the plain pick, Z = sum of w over the survivors and A(t) = sum of w over
//      survivors with l <= t, a survivor is kept iff A(l) > (1 - p) Z.  A is a step function that rises only at logits of the row, so
//      the smallest key c with A(c) > (1 - p) Z — a second bisection, over [key(t_k), key(m)] — is the smallest kept logit.  When no key
//      qualifies (p = 0) the search ends at key(m): the group of the maximum is always kept.  Columns with equal logits share one fate.
//      A is an fp32 sum in ONE fixed order for every candidate (a thread's columns in order, then row_pick::block_sum's);
//      fp32 addition is monotone in each operand, so A is monotone in the candidate and the bisection is well
//      defined.  Its error against float64 is a few 1e-7 of Z.
//   4. the pick: row_pick::inverse_cdf_pick, as in sample_rows_kernel, over w' = (l >= cut ? w : 0).  Unkept columns weigh exactly 0 and
//      are never picked; a NaN column fails l >= cut and weighs 0 too (it does not poison the sums here).
// Every block reduction is deterministic (no atomics), so the same row, u, T, k and p give the same token and cut on every launch, for
// every alignment of the row and whatever rows share the launch.
// Registers: up to 32768 columns the logits stay in registers through both descents, with the survivors' weights beside them in step 3;
// wider rows are read again from L2 in every round and step 3 evaluates the weights again.
// (A device function of the block's row as sample_row is: u, out, kept and cut point at the row's own entries, the last three nullable.)
template <int K, bool KEEP>
__device__ __forceinline__ void filtered_row(const float* __restrict__ r, int cols, float inv_t, int top_k, float top_p, const float* __restrict__ u,
                                             int64_t* __restrict__ out, int* __restrict__ kept, float* __restrict__ cut) {
  __shared__ float red[16];
  __shared__ unsigned red2[2][16];
  const int tid = threadIdx.x;
  const bool wide = starts_on_16_bytes(r);
  auto piece = [&](int k) { return load_piece(r, wide, cols, __uint_as_float(0x7fc00000u), k); };      // columns at or past `cols`: NaN, below every threshold
  int phase = 0;

  float4 v[KEEP ? K : 1];                    // KEEP: the logits, through both descents
  auto row = [&](int k) { return KEEP ? v[KEEP ? k : 0] : piece(k); };
  constexpr int UN = unroll_of(K, KEEP);
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float4 p = piece(k);
    if constexpr (KEEP) v[k] = p;
    m = fmaxf(m, piece_max(p));
  }
  m = block_max(m, red);
  if (!(m > -INFINITY)) {                    // nothing to keep (block-uniform)
    if (tid == 0) {
      if (out) *out = 0;
      if (kept) *kept = 0;
      if (cut) *cut = INFINITY;
    }
    return;
  }

  auto count_ge = [&](float c) {
    int n = 0;
#pragma unroll UN
    for (int k = 0; k < K; ++k) {
      const float4 p = row(k);
      n += (p.x >= c) + (p.y >= c) + (p.z >= c) + (p.w >= c);
    }
    return block_sum(n, red2, phase);
  };
  auto min_ge = [&](float c) {               // the smallest logit at or above c
    float s = INFINITY;
#pragma unroll UN
    for (int k = 0; k < K; ++k) {
      const float4 p = row(k);
      s = fminf(s, p.x >= c ? p.x : INFINITY); s = fminf(s, p.y >= c ? p.y : INFINITY);
      s = fminf(s, p.z >= c ? p.z : INFINITY); s = fminf(s, p.w >= c ? p.w : INFINITY);
    }
    return block_fmin(s, red2, phase);
  };

  // ---- top-k ----
  const int nvalid = count_ge(-INFINITY);    // the non-NaN columns (>= 1: the maximum)
  const int k_eff = (top_k > 0 && top_k < cols) ? min(top_k, nvalid) : nvalid;
  unsigned lo = KEY_NEG_INF, hi = float_key(m) + 1u;      // count(lo) >= k_eff > count(hi); float_key(m) <= key(+inf) = 0xff800000
  if (k_eff < nvalid) {
    while (hi - lo > 1u) {
      const unsigned mid = lo + (hi - lo) / 2u;
      const int n = count_ge(key_float(mid));
      if (n >= k_eff) {
        lo = mid;
        if (n == k_eff) break;
      } else {
        hi = mid;
      }
    }
  }
  const float t_k = min_ge(key_float(lo));
  float cutv = t_k;

  // columns at or past `cols` weigh 0 (sample_rows_kernel's weight, has_max holding here)
  auto weight = [&](float l, int i) { return i < cols ? temperature_weight(l, m, inv_t) : 0.f; };
  auto weights_ge = [&](float4 p, int k, float t) {      // the weights of piece k's columns at or above t, 0 elsewhere
    const int i = piece_column(k);
    p.x = p.x >= t ? weight(p.x, i) : 0.f; p.y = p.y >= t ? weight(p.y, i + 1) : 0.f;
    p.z = p.z >= t ? weight(p.z, i + 2) : 0.f; p.w = p.w >= t ? weight(p.w, i + 3) : 0.f;
    return p;
  };

  // ---- top-p over the survivors ----
  if (top_p < 1.f) {
    float4 ws[KEEP ? K : 1];
    float z = 0.f;
#pragma unroll UN
    for (int k = 0; k < K; ++k) {
      const float4 w = weights_ge(row(k), k, t_k);
      if constexpr (KEEP) ws[k] = w;
      z += ((w.x + w.y) + w.z) + w.w;
    }
    const float thr = (1.f - top_p) * block_sum(z, red2, phase);
    unsigned plo = float_key(t_k), phi = float_key(m);
    while (plo < phi) {
      const unsigned mid = plo + (phi - plo) / 2u;
      const float c = key_float(mid);
      float a = 0.f;
#pragma unroll UN
      for (int k = 0; k < K; ++k) {
        const float4 p = row(k), w = KEEP ? ws[KEEP ? k : 0] : weights_ge(p, k, t_k);
        a += (((p.x <= c ? w.x : 0.f) + (p.y <= c ? w.y : 0.f)) + (p.z <= c ? w.z : 0.f)) + (p.w <= c ? w.w : 0.f);
      }
      if (block_sum(a, red2, phase) > thr) phi = mid; else plo = mid + 1u;
    }
    cutv = min_ge(fmaxf(key_float(plo), t_k));
  }
  const int nkept = count_ge(cutv);
  if (tid == 0) {
    if (kept) *kept = nkept;
    if (cut) *cut = cutv;
  }
  if (out == nullptr) return;                // (block-uniform: the launch that only reports kept / cut)

  inverse_cdf_pick<K, KEEP>([&](int k) { return weights_ge(row(k), k, cutv); }, u, cols, out);
}
template <int K, bool KEEP>
__global__ __launch_bounds__(1024) void sample_filtered_kernel(const float* __restrict__ x, int64_t ld, int cols, float inv_t, int top_k, float top_p,
                                                               const float* __restrict__ u, int64_t* __restrict__ out, int* __restrict__ kept,
                                                               float* __restrict__ cut) {
  const int64_t b = blockIdx.x;
  filtered_row<K, KEEP>(x + b * ld, cols, inv_t, top_k, top_p, u + b, out ? out + b : nullptr, kept ? kept + b : nullptr, cut ? cut + b : nullptr);
}

// The greedy row in the same geometry: *out = the first column holding the row's maximum (mp_argmax_rows_f32's token: NaN columns never
// win, ties go to the smallest index), and 0 for a row without a non-NaN column, the sampling kernels' rule for a row with nothing to pick.
// Integer compares only: no order to fix.
template <int K, bool KEEP>
__device__ __forceinline__ void greedy_row(const float* __restrict__ r, int cols, int64_t* __restrict__ out) {
  __shared__ float red[16];
  __shared__ unsigned red2[2][16];
  const bool wide = starts_on_16_bytes(r);
  auto piece = [&](int k) { return load_piece(r, wide, cols, -INFINITY, k); };
  int phase = 0;
  float4 v[KEEP ? K : 1];
  constexpr int UN = unroll_of(K, KEEP);
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float4 p = piece(k);
    if constexpr (KEEP) v[k] = p;
    m = fmaxf(m, piece_max(p));
  }
  m = block_max(m, red);                     // (never NaN: fmaxf drops them; -inf for a row of NaN, which no column equals)
  int first = 0x7fffffff;
#pragma unroll UN
  for (int k = 0; k < K; ++k) {
    const float4 p = KEEP ? v[KEEP ? k : 0] : piece(k);
    const int i = piece_column(k);           // (the padding past `cols` is -inf too: the bound keeps it out of an all -inf row's pick)
    if (p.w == m && i + 3 < cols) first = min(first, i + 3);
    if (p.z == m && i + 2 < cols) first = min(first, i + 2);
    if (p.y == m && i + 1 < cols) first = min(first, i + 1);
    if (p.x == m && i < cols) first = min(first, i);
  }
  first = block_all_reduce(first, 0x7fffffff, [](int a, int b) { return min(a, b); }, red2, phase);
  if (threadIdx.x == 0) *out = first != 0x7fffffff ? first : 0;
}

// One launch for rows that each bring their own parameters (a batch group's requests): block b reads inv_t[b], top_k[b], top_p[b] from
// device memory and runs the body of the entry point that serves them on its row alone — greedy_row (inv_t = 0), sample_row (filters off) or
// filtered_row — so its token has that entry point's bits.  The branch is block-uniform (the values are made scalar first).  A row whose
// parameters no entry point accepts writes token 0 and ORs MP_POS_ERR_PICK into *err (the error word's own atomic OR, as every kernel that
// sets it; the picks use none); the other rows do not notice.
template <int K, bool KEEP>
__global__ __launch_bounds__(1024) void pick_rows_kernel(const float* __restrict__ x, int64_t ld, int cols, const float* __restrict__ inv_t_rows,
                                                         const int* __restrict__ top_k_rows, const float* __restrict__ top_p_rows,
                                                         const float* __restrict__ u, int64_t* __restrict__ out, int* __restrict__ err) {
  const int64_t b = blockIdx.x;
  const float inv_t = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(inv_t_rows[b])));
  const float top_p = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(top_p_rows[b])));
  const int top_k = __builtin_amdgcn_readfirstlane(top_k_rows[b]);
  const float* r = x + b * ld;
  if (!(inv_t >= 0.f && inv_t <= 3.402823466e38f) || !(top_p >= 0.f && top_p <= 1.f) || top_k < 0) {      // (NaN fails both compares)
    if (threadIdx.x == 0) {
      out[b] = 0;
      atomicOr(err, MP_POS_ERR_PICK);
    }
    return;
  }
  if (inv_t == 0.f) greedy_row<K, KEEP>(r, cols, out + b);
  else if (!(top_k > 0 && top_k < cols) && top_p >= 1.f) sample_row<K, KEEP>(r, cols, inv_t, u + b, out + b);
  else filtered_row<K, KEEP>(r, cols, inv_t, top_k, top_p, u + b, out + b, nullptr, nullptr);
}

}  // namespace

extern "C" int mp_sample_rows_f32(const float* logits, int64_t ld, int64_t rows, int cols, float inv_temperature, const float* u, int64_t* out,
                                  hipStream_t stream) {
  MP_REQUIRE(cols > 0 && cols <= 65536 && rows >= 0, MP_ERR_SHAPE, "mp_sample_rows_f32: bad shape (rows=%lld cols=%d; 0 < cols <= 65536)",
             (long long)rows, cols);
  MP_REQUIRE(inv_temperature > 0.f && inv_temperature <= 3.402823466e38f, MP_ERR_SHAPE, "mp_sample_rows_f32: inv_temperature=%g must be positive and finite",
             (double)inv_temperature);
  if (rows == 0) return MP_OK;
  MP_REQUIRE(logits != nullptr && u != nullptr && out != nullptr, MP_ERR_ARG, "mp_sample_rows_f32: null operand");
  MP_REQUIRE(rows == 1 || ld >= cols || ld == 0, MP_ERR_SHAPE, "mp_sample_rows_f32: ld=%lld < cols=%d (ld = 0: one row against every u)",
             (long long)ld, cols);
  for_width(cols, [&](auto shape) {
    using S = decltype(shape);
    hipLaunchKernelGGL((sample_rows_kernel<S::K, S::KEEP>), dim3((unsigned)rows), dim3(1024), 0, stream, logits, ld, cols, inv_temperature, u, out);
  });
  return mp_check_launch("mp_sample_rows_f32");
}

extern "C" int mp_sample_filtered_rows_f32(const float* logits, int64_t ld, int64_t rows, int cols, float inv_temperature, int top_k, float top_p,
                                           const float* u, int64_t* out, int* kept, float* cut, hipStream_t stream) {
  MP_REQUIRE(cols > 0 && cols <= 65536 && rows >= 0, MP_ERR_SHAPE, "mp_sample_filtered_rows_f32: bad shape (rows=%lld cols=%d; 0 < cols <= 65536)",
             (long long)rows, cols);
  MP_REQUIRE(inv_temperature > 0.f && inv_temperature <= 3.402823466e38f, MP_ERR_SHAPE,
             "mp_sample_filtered_rows_f32: inv_temperature=%g must be positive and finite", (double)inv_temperature);
  MP_REQUIRE(top_p >= 0.f && top_p <= 1.f, MP_ERR_SHAPE, "mp_sample_filtered_rows_f32: top_p=%g must lie in [0, 1]", (double)top_p);
  MP_REQUIRE(top_k >= 0, MP_ERR_SHAPE, "mp_sample_filtered_rows_f32: top_k=%d must not be negative (0: no top-k)", top_k);
  if (rows == 0) return MP_OK;
  MP_REQUIRE(logits != nullptr && u != nullptr && out != nullptr, MP_ERR_ARG, "mp_sample_filtered_rows_f32: null operand");
  MP_REQUIRE(rows == 1 || ld >= cols || ld == 0, MP_ERR_SHAPE, "mp_sample_filtered_rows_f32: ld=%lld < cols=%d (ld = 0: one row against every u)",
             (long long)ld, cols);
  int64_t* tok = out;
  if (!(top_k > 0 && top_k < cols) && top_p >= 1.f) {      // filters off: the plain pick's token, bit for bit, from the plain pick itself
    const int rc = mp_sample_rows_f32(logits, ld, rows, cols, inv_temperature, u, out, stream);
    if (rc != MP_OK || (kept == nullptr && cut == nullptr)) return rc;
    tok = nullptr;                           // a second launch, only for a caller that asks for kept / cut: it writes those two alone
  }
  for_width(cols, [&](auto shape) {
    using S = decltype(shape);
    hipLaunchKernelGGL((sample_filtered_kernel<S::K, S::KEEP>), dim3((unsigned)rows), dim3(1024), 0, stream, logits, ld, cols, inv_temperature, top_k,
                       top_p, u, tok, kept, cut);
  });
  return mp_check_launch("mp_sample_filtered_rows_f32");
}

extern "C" int mp_pick_rows_f32(const float* logits, int64_t ld, int64_t rows, int cols, const float* inv_temperature, const int* top_k,
                                const float* top_p, const float* u, int64_t* out, int* err, hipStream_t stream) {
  MP_REQUIRE(cols > 0 && cols <= 65536 && rows >= 0, MP_ERR_SHAPE, "mp_pick_rows_f32: bad shape (rows=%lld cols=%d; 0 < cols <= 65536)",
             (long long)rows, cols);
  MP_REQUIRE(rows <= 1 || ld >= cols, MP_ERR_SHAPE, "mp_pick_rows_f32: ld=%lld < cols=%d", (long long)ld, cols);
  if (rows == 0) return MP_OK;
  MP_REQUIRE(logits != nullptr && inv_temperature != nullptr && top_k != nullptr && top_p != nullptr && u != nullptr && out != nullptr &&
                 err != nullptr, MP_ERR_ARG, "mp_pick_rows_f32: null operand");
  for_width(cols, [&](auto shape) {
    using S = decltype(shape);
    hipLaunchKernelGGL((pick_rows_kernel<S::K, S::KEEP>), dim3((unsigned)rows), dim3(1024), 0, stream, logits, ld, cols, inv_temperature, top_k,
                       top_p, u, out, err);
  });
  return mp_check_launch("mp_pick_rows_f32");
}
