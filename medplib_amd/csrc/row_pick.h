// The shared core of the kernels that pick columns of an fp32 row held by one block of 1024 threads: the temperature pick and its top-k / top-p
// form (sampling.hip) and the beam step's row top-2nb (beam_search.hip).  gfx950, wave64.
#pragma once
#include "common.h"

namespace row_pick {

// ---- geometry ----
// One block of BLOCK threads per row, K float4 pieces per thread: piece p = tid + k * BLOCK covers columns 4p .. 4p + 3, so a wave's 64 pieces
// are 1 KB of consecutive columns.  Up to HELD_COLS columns (K = 8: the decode row, 32000 + added tokens) the row stays in registers after
// the one read (KEEP); 16 pieces per thread do not fit the 128 registers of a 1024-thread block, so wider rows (K = 16, up to MAX_COLS) are
// read again from L2 by every pass, UN pieces in flight (four, not sixteen).
constexpr int BLOCK = 1024;
constexpr int HELD_COLS = 4 * BLOCK * 8, MAX_COLS = 4 * BLOCK * 16;
constexpr int unroll_of(int K, bool KEEP) { return KEEP ? K : 4; }

template <int K_, bool KEEP_>
struct Shape {
  static constexpr int K = K_;
  static constexpr bool KEEP = KEEP_;
};
// launch(Shape<K, KEEP>{}) for a row of `cols` columns (0 < cols <= MAX_COLS, checked by the caller)
template <typename F>
inline void for_width(int cols, F&& launch) {
  if (cols <= HELD_COLS) launch(Shape<8, true>{});
  else launch(Shape<16, false>{});
}

__device__ __forceinline__ int piece_column(int k) { return 4 * ((int)threadIdx.x + k * BLOCK); }      // the first column of this thread's piece k

// The pieces of one row: one 16-byte load per piece when the row starts on 16 bytes — the decode row does — and four 4-byte loads at a
// 16-byte lane stride otherwise, over the same 1 KB per wave.  A row that does not start on 16 bytes (rows of a batch with an odd ld) is read
// column by column into the SAME registers: a unit-stride read over the lanes would change which thread sums which columns, and with it the
// last bits of every sum.  Columns at or past `cols` are `pad`.
__device__ __forceinline__ bool starts_on_16_bytes(const float* row) { return (reinterpret_cast<uintptr_t>(row) & 15) == 0; }      // (block-uniform)
__device__ __forceinline__ float4 load_piece(const float* r, bool wide, int cols, float pad, int k) {
  const int i = piece_column(k);
  float4 p;
  if (wide && i + 3 < cols) {
    p = *reinterpret_cast<const float4*>(r + i);
  } else {                                   // the piece that straddles `cols`, pieces past it, and rows off 16 bytes
    p.x = i < cols ? r[i] : pad;
    p.y = i + 1 < cols ? r[i + 1] : pad;
    p.z = i + 2 < cols ? r[i + 2] : pad;
    p.w = i + 3 < cols ? r[i + 3] : pad;
  }
  return p;
}
__device__ __forceinline__ float piece_max(float4 p) { return fmaxf(fmaxf(p.x, p.y), fmaxf(p.z, p.w)); }      // (fmaxf drops NaN)

// ---- block all-reduce with ONE barrier ----
// The xor tree over the lanes (offsets 32, 16, ... 1), the 16 wave results to one of two LDS slots in turn (slot = red[phase], phase flips per
// call), then identity (op) s[0] (op) ... (op) s[15] in index order in every thread: one fixed order, so an fp32 sum has the same bits on
// every launch.  One barrier is enough: a thread can only be two reductions ahead of the slowest after passing the barrier of the one
// between, so the slot it writes has been read by everyone.  `phase` is a per-thread value that every thread of the block advances alike:
// every call must be reached by the whole block.  W is the LDS word of T's size, so that reductions of different 32-bit types share the slots.
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int o) {
  const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ int lane_xor(int v, int o) { return __shfl_xor(v, o, 64); }
__device__ __forceinline__ float lane_xor(float v, int o) { return __shfl_xor(v, o, 64); }
__device__ __forceinline__ unsigned long long lane_xor(unsigned long long v, int o) { return shfl_xor_u64(v, o); }

template <typename T, typename W, typename Op>
__device__ __forceinline__ T block_all_reduce(T v, T identity, Op op, W (*red)[16], int& phase) {
  static_assert(sizeof(T) == sizeof(W), "the LDS word must have the value's size");
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, lane_xor(v, o));
  W* s = red[phase];
  phase ^= 1;
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = __builtin_bit_cast(W, v);
  __syncthreads();
  T t = identity;
#pragma unroll
  for (int i = 0; i < 16; ++i) t = op(t, __builtin_bit_cast(T, s[i]));
  return t;
}
template <typename T, typename W>
__device__ __forceinline__ T block_sum(T v, W (*red)[16], int& phase) {
  return block_all_reduce(v, T(0), [](T a, T b) { return a + b; }, red, phase);
}
template <typename W>
__device__ __forceinline__ float block_fmin(float v, W (*red)[16], int& phase) {
  return block_all_reduce(v, INFINITY, [](float a, float b) { return fminf(a, b); }, red, phase);
}
template <typename W>
__device__ __forceinline__ float block_fmax(float v, W (*red)[16], int& phase) {
  return block_all_reduce(v, -INFINITY, [](float a, float b) { return fmaxf(a, b); }, red, phase);
}

// ---- the order-preserving unsigned image of a float ----
// sign-magnitude -> unsigned: a < b as floats iff key(a) < key(b) as integers, -0 below +0; every integer step is one float step.
constexpr unsigned KEY_NEG_INF = 0x007fffffu;      // float_key(-inf)
__device__ __forceinline__ unsigned float_key(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_float(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// ---- the inverse-CDF pick ----
__device__ __forceinline__ float lane_scan_step(float v, int o, int lane) {
  const float t = __shfl_up(v, o, 64);
  return lane >= o ? v + t : v;
}

// *out = the smallest column i with w_i > 0 whose cumulative weight C(i) exceeds *u * C(last column), for the block's row; weights(k) yields
// the four weights of this thread's piece k (the same bits whenever it is asked again; 0 at or past the row's end) and is all that
// tells the callers apart.  Reached by the whole block (three barriers); thread 0 writes.
//   1. the sum of every piece in a fixed order ((w0 + w1) + w2) + w3, an inclusive scan of the 64 piece sums of every (k, wave) chunk
//      (Hillis-Steele over the lanes, offsets 1, 2, ... 32), the 16 K chunk totals scanned by wave 0 (16 K / 64 consecutive chunks per lane,
//      then the lane scan) — the cumulative weight in front of every piece;
//   2. C(i) = (chunk base + lane base) + the piece's running sum.  Every thread compares the C of its own columns with the target, which is
//      the scan inside the chunk that holds the target without reading the row again: the pieces of every other chunk lie wholly on one side
//      of the target and yield no candidate (up to the rounding of C, below).  The block takes the smallest candidate.
// No atomics and no order that depends on timing: the same weights and u give the same column on every launch, whatever rows share it.
// C is an fp32 sum whose grouping changes at piece, lane and chunk borders, so it may dip by an ulp of the total at such a border; "smallest i
// with C(i) > target and w_i > 0" is well defined all the same, and every i in front of the pick has C(i) <= target.  If no column qualifies
// (u >= 1 — the keyed generator does return exactly 1.0, see include/medplib_hip.h — or u so close to 1 that rounding leaves the last C at or
// below the target; also a NaN u, or a NaN weight, which makes C NaN from there on) the pick is the LAST column with w > 0; u <= 0 gives the
// first.  A row without any w > 0 gives 0.
// KEEP: the weights and the lane scans stay in registers between the two steps; otherwise step 2 evaluates them again (the same expressions
// on the same weights: the same bits).
template <int K, bool KEEP, typename Weights>
__device__ __forceinline__ void inverse_cdf_pick(Weights&& weights, const float* __restrict__ u, int cols, int64_t* __restrict__ out) {
  constexpr int NC = 16 * K, UN = unroll_of(K, KEEP);      // chunks of 64 pieces (256 columns): chunk c = k * 16 + wave, in column order
  __shared__ float chunk_sum[NC];            // totals, then the cumulative weight in front of each chunk
  __shared__ float total_s;
  __shared__ int first_s[16], last_s[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  auto lane_scan = [&](float4 w) {           // inclusive scan of the piece sums over the lanes of this wave's chunk
    float inc = ((w.x + w.y) + w.z) + w.w;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) inc = lane_scan_step(inc, o, lane);
    return inc;
  };
  float4 held[KEEP ? K : 1];
  float incl[KEEP ? K : 1];
  if constexpr (KEEP) {                      // the K scans interleaved (offset outer, k inner): the same bits, K independent shuffles in flight
                                             // (piece by piece, as below, the plain pick is 0.25 us slower on the decode row)
#pragma unroll
    for (int k = 0; k < K; ++k) {
      held[k] = weights(k);
      incl[k] = ((held[k].x + held[k].y) + held[k].z) + held[k].w;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
      for (int k = 0; k < K; ++k) incl[k] = lane_scan_step(incl[k], o, lane);
    }
    if (lane == 63) {
#pragma unroll
      for (int k = 0; k < K; ++k) chunk_sum[k * 16 + wave] = incl[k];
    }
  } else {
#pragma unroll UN
    for (int k = 0; k < K; ++k) {
      const float inc = lane_scan(weights(k));
      if (lane == 63) chunk_sum[k * 16 + wave] = inc;
    }
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
  const float target = *u * total_s;

  int first = 0x7fffffff, last = -1;         // smallest qualifying column of this thread; its last column with w > 0
#pragma unroll UN
  for (int k = 0; k < K; ++k) {
    const float4 w = KEEP ? held[KEEP ? k : 0] : weights(k);
    float prev = __shfl_up(KEEP ? incl[KEEP ? k : 0] : lane_scan(w), 1, 64);
    if (lane == 0) prev = 0.f;
    const float base = chunk_sum[k * 16 + wave] + prev;
    const int i = piece_column(k);
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
    *out = min(first != 0x7fffffff ? first : (last >= 0 ? last : 0), cols - 1);      // (the clamp never binds: w = 0 past cols)
  }
}

}  // namespace row_pick
