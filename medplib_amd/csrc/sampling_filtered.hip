// Top-k / top-p truncation of the next-token distribution in front of the temperature pick of sampling.hip (HF 4.31's warper chain
// TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> multinomial, what the reference's vqa_infer.py:430-442 asks of
// generate(do_sample=True, temperature=, top_p=)).  gfx950, wave64.
#include "common.h"

extern "C" int mp_sample_rows_f32(const float* logits, int64_t ld, int64_t rows, int cols, float inv_temperature, const float* u, int64_t* out,
                                  hipStream_t stream);

namespace {

// One block of 1024 threads per row, the row in registers in the piece layout of sample_rows_kernel (sampling.hip: piece p = tid + k * 1024
// covers columns 4p .. 4p + 3).  The truncation is a threshold on the logit, `cut`: a column is kept iff l >= cut.
//   1. row maximum m; a row without one above -inf (all -inf, all NaN) keeps nothing: token 0, kept 0, cut +inf.
//   2. top-k: t_k = the k-th largest logit counting multiplicity, found by bisection on the order-preserving integer key of a float
//      (sign-magnitude -> unsigned) over [key(-inf), key(m)]: every round counts the columns with l >= candidate over the block.  The count
//      is an integer and the compare is on the logits themselves, so the selection is exact and ties at t_k all survive.  The descent
//      stops early at a candidate that exactly k columns reach; t_k is then the smallest of those.  NaN columns (and the padding past
//      `cols`, loaded as NaN) compare false and never count.  Without top-k, t_k = the smallest non-NaN logit.
//   3. top-p over the survivors {l >= t_k}: with w the weights of sampling.hip, Z = sum of w over the survivors and A(t) = sum of w over
//      survivors with l <= t, a survivor is kept iff A(l) > (1 - p) Z.  A is a step function that rises only at logits of the row, so
//      the smallest key c with A(c) > (1 - p) Z — a second bisection, over [key(t_k), key(m)] — is the smallest kept logit.  When no key
//      qualifies (p = 0) the search ends at key(m): the group of the maximum is always kept.  Columns with equal logits share one fate.
//      A is an fp32 sum in ONE fixed order for every candidate (a thread's columns in order, the xor tree over the lanes, the 16 wave
//      sums in index order); fp32 addition is monotone in each operand, so A is monotone in the candidate and the bisection is well
//      defined.  Its error against float64 is a few 1e-7 of Z.
//   4. the pick: steps 2 and 3 of sample_rows_kernel, the same expressions in the same order, over w' = (l >= cut ? w : 0).  Unkept columns
//      weigh exactly 0 and are never picked; a NaN column fails l >= cut and weighs 0 too (it does not poison the sums here).
// Every block reduction is deterministic (no atomics), so the same row, u, T, k and p give the same token and cut on every launch, for
// every alignment of the row and whatever rows share the launch.  The reductions of the descents take ONE barrier each: the 16 wave
// results go to one of two LDS slots in turn, and a thread can only be two reductions ahead of the slowest after passing the barrier
// of the one between.
// Registers: up to 32768 columns (K = 8, the decode row) the logits stay in registers through both descents, with the survivors' weights
// beside them in step 3.  Wider rows (K = 16) do not fit the 128 registers of a 1024-thread block, as in sample_rows_kernel<16, false>:
// every round reads the row again from L2 and step 3 evaluates the weights again.
constexpr unsigned KEY_NEG_INF = 0x007fffffu;      // key_of(-inf)

__device__ __forceinline__ unsigned key_of(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float float_of(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ float lane_scan_step(float v, int o, int lane) {
  const float t = __shfl_up(v, o, 64);
  return lane >= o ? v + t : v;
}

// block all-reduces with one barrier: slot = red[phase], phase flips per call (see above)
__device__ __forceinline__ int block_count(int v, unsigned (*red)[16], int& phase) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  unsigned* s = red[phase];
  phase ^= 1;
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = (unsigned)v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) t += (int)s[i];
  return t;
}
__device__ __forceinline__ float block_fsum(float v, unsigned (*red)[16], int& phase) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  unsigned* s = red[phase];
  phase ^= 1;
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = __float_as_uint(v);
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) t += __uint_as_float(s[i]);
  return t;
}
__device__ __forceinline__ float block_fmin(float v, unsigned (*red)[16], int& phase) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  unsigned* s = red[phase];
  phase ^= 1;
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = __float_as_uint(v);
  __syncthreads();
  float t = __uint_as_float(s[0]);
#pragma unroll
  for (int i = 1; i < 16; ++i) t = fminf(t, __uint_as_float(s[i]));
  return t;
}

template <int K, bool KEEP>
__global__ __launch_bounds__(1024) void sample_filtered_kernel(const float* __restrict__ x, int64_t ld, int cols, float inv_t, int top_k, float top_p,
                                                               const float* __restrict__ u, int64_t* __restrict__ out, int* __restrict__ kept,
                                                               float* __restrict__ cut) {
  constexpr int NC = 16 * K;                 // chunks of 64 pieces (256 columns): chunk c = k * 16 + wave, in column order
  __shared__ float red[16];
  __shared__ unsigned red2[2][16];
  __shared__ float chunk_sum[NC];            // totals, then the cumulative weight in front of each chunk
  __shared__ float total_s;
  __shared__ int first_s[16], last_s[16];
  const float* r = x + (int64_t)blockIdx.x * ld;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool wide = (reinterpret_cast<uintptr_t>(r) & 15) == 0;       // (block-uniform)
  const float pad = __uint_as_float(0x7fc00000u);                     // columns at or past `cols`: NaN, below every threshold
  int phase = 0;

  auto piece = [&](int k) {
    const int i = 4 * (tid + k * 1024);
    float4 p;
    if (wide && i + 3 < cols) {
      p = *reinterpret_cast<const float4*>(r + i);
    } else {                                 // the piece that straddles `cols`, pieces past it, and rows off 16 bytes
      p.x = i < cols ? r[i] : pad;
      p.y = i + 1 < cols ? r[i + 1] : pad;
      p.z = i + 2 < cols ? r[i + 2] : pad;
      p.w = i + 3 < cols ? r[i + 3] : pad;
    }
    return p;
  };
  float4 v[KEEP ? K : 1];                    // KEEP: the logits, through both descents
  auto row = [&](int k) { return KEEP ? v[KEEP ? k : 0] : piece(k); };
  constexpr int UN = KEEP ? K : 4;           // (re-read rows: four pieces in flight, not sixteen)
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float4 p = piece(k);
    if constexpr (KEEP) v[k] = p;
    m = fmaxf(m, fmaxf(fmaxf(p.x, p.y), fmaxf(p.z, p.w)));      // (fmaxf drops NaN)
  }
  m = block_max(m, red);
  if (!(m > -INFINITY)) {                    // nothing to keep (block-uniform)
    if (tid == 0) {
      if (out) out[blockIdx.x] = 0;
      if (kept) kept[blockIdx.x] = 0;
      if (cut) cut[blockIdx.x] = INFINITY;
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
    return block_count(n, red2, phase);
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
  unsigned lo = KEY_NEG_INF, hi = key_of(m) + 1u;      // count(lo) >= k_eff > count(hi); key_of(m) <= key(+inf) = 0xff800000
  if (k_eff < nvalid) {
    while (hi - lo > 1u) {
      const unsigned mid = lo + (hi - lo) / 2u;
      const int n = count_ge(float_of(mid));
      if (n >= k_eff) {
        lo = mid;
        if (n == k_eff) break;
      } else {
        hi = mid;
      }
    }
  }
  const float t_k = min_ge(float_of(lo));
  float cutv = t_k;

  // a column equal to the maximum has w = 1 exactly; columns at or past `cols` weigh 0 (sample_rows_kernel's weight, has_max holding here)
  auto weight = [&](float l, int i) { return i < cols ? (l == m ? 1.f : __expf((l - m) * inv_t)) : 0.f; };

  // ---- top-p over the survivors ----
  if (top_p < 1.f) {
    auto surv = [&](float4 p, int k) {       // the survivors' weights of piece k, 0 elsewhere
      const int i = 4 * (tid + k * 1024);
      p.x = p.x >= t_k ? weight(p.x, i) : 0.f; p.y = p.y >= t_k ? weight(p.y, i + 1) : 0.f;
      p.z = p.z >= t_k ? weight(p.z, i + 2) : 0.f; p.w = p.w >= t_k ? weight(p.w, i + 3) : 0.f;
      return p;
    };
    float4 ws[KEEP ? K : 1];
    float z = 0.f;
#pragma unroll UN
    for (int k = 0; k < K; ++k) {
      const float4 w = surv(row(k), k);
      if constexpr (KEEP) ws[k] = w;
      z += ((w.x + w.y) + w.z) + w.w;
    }
    const float thr = (1.f - top_p) * block_fsum(z, red2, phase);
    unsigned plo = key_of(t_k), phi = key_of(m);
    while (plo < phi) {
      const unsigned mid = plo + (phi - plo) / 2u;
      const float c = float_of(mid);
      float a = 0.f;
#pragma unroll UN
      for (int k = 0; k < K; ++k) {
        const float4 p = row(k), w = KEEP ? ws[KEEP ? k : 0] : surv(p, k);
        a += (((p.x <= c ? w.x : 0.f) + (p.y <= c ? w.y : 0.f)) + (p.z <= c ? w.z : 0.f)) + (p.w <= c ? w.w : 0.f);
      }
      if (block_fsum(a, red2, phase) > thr) phi = mid; else plo = mid + 1u;
    }
    cutv = min_ge(fmaxf(float_of(plo), t_k));
  }
  const int nkept = count_ge(cutv);
  if (tid == 0) {
    if (kept) kept[blockIdx.x] = nkept;
    if (cut) cut[blockIdx.x] = cutv;
  }
  if (out == nullptr) return;                // (block-uniform: the launch that only reports kept / cut)

  // ---- the pick of sample_rows_kernel over the kept columns ----
  auto weights = [&](float4 p, int k) {
    const int i = 4 * (tid + k * 1024);
    p.x = p.x >= cutv ? weight(p.x, i) : 0.f; p.y = p.y >= cutv ? weight(p.y, i + 1) : 0.f;
    p.z = p.z >= cutv ? weight(p.z, i + 2) : 0.f; p.w = p.w >= cutv ? weight(p.w, i + 3) : 0.f;
    return p;
  };
  auto lane_scan = [&](float4 w) {            // inclusive scan of the piece sums over the lanes of this wave's chunk
    float inc = ((w.x + w.y) + w.z) + w.w;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) inc = lane_scan_step(inc, o, lane);
    return inc;
  };
  float incl[KEEP ? K : 1];                  // KEEP: the scans stay too; otherwise the second pass repeats them (the same bits)
#pragma unroll UN
  for (int k = 0; k < K; ++k) {
    const float4 w = weights(row(k), k);
    const float inc = lane_scan(w);
    if constexpr (KEEP) { v[k] = w; incl[k] = inc; }
    if (lane == 63) chunk_sum[k * 16 + wave] = inc;
  }
  __syncthreads();
  if (wave == 0) {                           // NC / 64 consecutive chunks per lane, then a scan over the lanes
    constexpr int PER = NC / 64;
    float s[PER], run = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) { s[j] = chunk_sum[lane * PER + j]; run += s[j]; }
    float inc = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) inc = lane_scan_step(inc, o, lane);
    float base = __shfl_up(inc, 1, 64);      // the cumulative weight in front of this lane's chunks
    if (lane == 0) base = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) { chunk_sum[lane * PER + j] = base; base += s[j]; }
    if (lane == 63) total_s = inc;
  }
  __syncthreads();
  const float target = u[blockIdx.x] * total_s;

  int first = 0x7fffffff, last = -1;         // smallest qualifying column of this thread; its last column with w > 0
#pragma unroll UN
  for (int k = 0; k < K; ++k) {
    const float4 w = KEEP ? v[KEEP ? k : 0] : weights(piece(k), k);      // (the same expression on the same logits: the same bits as above)
    float prev = __shfl_up(KEEP ? incl[KEEP ? k : 0] : lane_scan(w), 1, 64);
    if (lane == 0) prev = 0.f;
    const float base = chunk_sum[k * 16 + wave] + prev;
    const int i = 4 * (tid + k * 1024);
    const float c0 = base + w.x, c1 = base + (w.x + w.y), c2 = base + ((w.x + w.y) + w.z), c3 = base + (((w.x + w.y) + w.z) + w.w);
    if (w.w > 0.f) { last = max(last, i + 3); if (c3 > target) first = min(first, i + 3); }
    if (w.z > 0.f) { last = max(last, i + 2); if (c2 > target) first = min(first, i + 2); }
    if (w.y > 0.f) { last = max(last, i + 1); if (c1 > target) first = min(first, i + 1); }
    if (w.x > 0.f) { last = max(last, i); if (c0 > target) first = min(first, i); }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    first = min(first, __shfl_xor(first, o, 64));
    last = max(last, __shfl_xor(last, o, 64));
  }
  if (lane == 0) { first_s[wave] = first; last_s[wave] = last; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 16; ++w) { first = min(first, first_s[w]); last = max(last, last_s[w]); }
    out[blockIdx.x] = min(first != 0x7fffffff ? first : (last >= 0 ? last : 0), cols - 1);      // (the clamp never binds: w = 0 past cols)
  }
}

}  // namespace

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
  if (cols <= 32768)
    hipLaunchKernelGGL((sample_filtered_kernel<8, true>), dim3((unsigned)rows), dim3(1024), 0, stream, logits, ld, cols, inv_temperature, top_k,
                       top_p, u, tok, kept, cut);
  else
    hipLaunchKernelGGL((sample_filtered_kernel<16, false>), dim3((unsigned)rows), dim3(1024), 0, stream, logits, ld, cols, inv_temperature, top_k,
                       top_p, u, tok, kept, cut);
  return mp_check_launch("mp_sample_filtered_rows_f32");
}
