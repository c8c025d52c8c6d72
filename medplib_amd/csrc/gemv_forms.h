// The three forms of the decode-step GEMV, y[m, n] = epilogue(x[m, :] . W[n, :]) for M <= 8 rows, written once over a weight-type policy:
// SHARED (one matrix for all rows), INDEXED (a matrix per row: MoE experts) and K-SPLIT (the narrow projections with a long K), and the host
// dispatch that chooses among them.  A decode step reads every weight once, so every form is bound by the HBM stream of W: a wave owns four
// output rows, streams them with 16-byte non-temporal loads against the x rows, reduces across the wave and applies the epilogues of
// gemv_epilogue.h.  The two policies (bf16 weights: gemv_bf16.hip; int8 codes with an fp32 scale per output row: gemv_w8.hip) differ in how a
// wave streams its four rows — each loop's shape was arrived at by measurement and is recorded at the loop — and in whether the finished sum is
// multiplied by the row's scale.  One rule for a capacity-dropped row (row_keep[m] < 0) of the indexed and K-split forms: it streams no weights;
// the plain forms store gv_store_dropped, the SwiGLU form leaves the row unwritten (nothing reads it).
#pragma once
#include "gemv_epilogue.h"

// MP_GEMV_KSPLIT=0: the one-wave-per-four-rows kernels instead of the K-split form (A/B), for either weight type.  Read once, at the first
// launch (outside the unnamed namespace: one copy for both entry points).
inline bool gv_ksplit_enabled() {
  static const bool on = [] { const char* e = getenv("MP_GEMV_KSPLIT"); return !(e && atoi(e) == 0); }();
  return on;
}

namespace {

constexpr int GV_MAXM = 8;
typedef __attribute__((ext_vector_type(4))) int i32x4;

template <class T>
struct GemvArgsT {
  const bf16_t* x; int64_t ldx;
  const T* W; int64_t ldw; int64_t strideW;       // [N, K] or [E, N, K]
  void* y; int64_t ldy;
  const float* bias; const bf16_t* residual; int64_t ldr;
  const int* w_index;        // [M] device: weight matrix per row (null = one shared matrix)
  const float* row_scale;    // [M] device or null
  const int* row_keep;       // [M] device or null: rows with row_keep[m] < 0 are capacity-dropped tokens (gv_store_dropped)
  int M, N, K, act, out_f32;
  float alpha;
  const float* scale; int64_t strideScale;        // int8 codes: one scale per output row, [N] or [E, N] (bf16: null, 0)
};
using GemvArgs = GemvArgsT<bf16_t>;

// The weight stream: every byte is read once per token by ONE wave, so the loads are marked non-temporal (streaming lines do not displace
// the x rows, norm weights and KV cache other kernels of the decode step re-read from L2; MP_GEMV_NT=0 at build time restores the default
// policy for an A/B).
#ifndef MP_GEMV_NT
#define MP_GEMV_NT 1
#endif
__device__ __forceinline__ bf16x8 gv_ldw(const bf16_t* p) {
#if MP_GEMV_NT
  return __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(p));
#else
  return *reinterpret_cast<const bf16x8*>(p);
#endif
}

__device__ __forceinline__ float gv_dot8(const bf16x8 a, const bf16x8 b, float acc) {
#pragma unroll
  for (int j = 0; j < 8; ++j) acc = fmaf((float)a[j], (float)b[j], acc);
  return acc;
}

__device__ __forceinline__ i32x4 gq_ldw(const int8_t* p) { return __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(p)); }

struct X16 { bf16x8 a, b; };                                  // the sixteen x values against one 16-byte load of codes
__device__ __forceinline__ X16 gq_ldx(const bf16_t* p) { return X16{*reinterpret_cast<const bf16x8*>(p), *reinterpret_cast<const bf16x8*>(p + 8)}; }

// One 16-byte load of each of the wave's four W rows against the sixteen x values of each of the M rows: one convert per weight, one FMA per
// weight and row (the compiler pairs the four rows' FMAs into packed ones), ascending k in every (row of x, row of W) chain.
template <int M>
__device__ __forceinline__ void gq_fma16(const X16 (&x)[M], const i32x4 (&w)[4], float (&acc)[M][4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float c[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int b = 0; b < 4; ++b) c[r][b] = (float)(int8_t)(w[r][q] >> (8 * b));
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const float xf = (float)(q < 2 ? x[m].a[(q & 1) * 4 + b] : x[m].b[(q & 1) * 4 + b]);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[m][r] = fmaf(c[r][b], xf, acc[m][r]);
      }
  }
}

// The weight stream of one wave over int8 codes: the steps k, k + kstep, ... < K of its four code rows against M rows of x (x + m * ldx), one
// step of 4 x 16 bytes per lane per trip with the NEXT step requested before this one is multiplied, so four to eight weight loads per lane
// are in flight all the way.  A trip is one step, not the bf16 stream's two: the compiler converts a trip's codes to fp32 up front whatever the
// source order (scheduling barriers do not hold it back), and two steps' worth is 128 floats: 232 VGPRs in the one-row kernel and spills in the
// sixteen-wave one, against ~110 VGPRs and four waves per SIMD here.  acc[m][r] += this lane's share; sums in ascending k.
template <int M>
__device__ __forceinline__ void gq_stream(const bf16_t* __restrict__ x, int64_t ldx, const int8_t* const (&wp)[4], int k, int kstep, int K,
                                          float (&acc)[M][4]) {
  if (k >= K) return;
  i32x4 w[4];
  X16 xs[M];
#pragma unroll
  for (int r = 0; r < 4; ++r) w[r] = gq_ldw(wp[r] + k);
#pragma unroll
  for (int m = 0; m < M; ++m) xs[m] = gq_ldx(x + (int64_t)m * ldx + k);
#pragma unroll 1
  for (; k < K; k += kstep) {
    i32x4 wn[4] = {w[0], w[1], w[2], w[3]};
    X16 xn[M];
#pragma unroll
    for (int m = 0; m < M; ++m) xn[m] = xs[m];
    if (k + kstep < K) {
#pragma unroll
      for (int r = 0; r < 4; ++r) wn[r] = gq_ldw(wp[r] + k + kstep);
#pragma unroll
      for (int m = 0; m < M; ++m) xn[m] = gq_ldx(x + (int64_t)m * ldx + k + kstep);
    }
    gq_fma16<M>(xs, w, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) w[r] = wn[r];
#pragma unroll
    for (int m = 0; m < M; ++m) xs[m] = xn[m];
  }
}

// ---------------- the weight policies: element type, whether a finished sum takes the row's scale, and the three streams ----------------
// shared_dot: this lane's share of x[m] . W[row r] for M rows, added into acc (no reduction).  row_dot / part_dot: one x row against the wave's
// four W rows — all of K, or K part kp (0..3) of the K-split form, the steps kp, kp + 4, ... — wave-reduced: acc[r] = (the part's share of) x . W[row r].
struct WeightBf16 {
  using elem = bf16_t;
  static constexpr bool SCALED = false;

  template <int M>
  static __device__ __forceinline__ void shared_dot(const bf16_t* x, int64_t ldx, const bf16_t* const (&wp)[4], int K, int lane,
                                                    float (&acc)[M][4]) {
    const int iters = K / 512;                                // 64 lanes x 8 elements per step
    int k = lane * 8;
    // (four steps per trip for the one-row case, 16 loads in flight, was measured too: o_proj 11.0 -> 11.2 us — no change)
    int it = 0;
    for (; it + 1 < iters; it += 2, k += 1024) {              // two steps per trip: 8 weight loads in flight per lane
      bf16x8 w0[4], w1[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) { w0[r] = gv_ldw(wp[r] + k); w1[r] = gv_ldw(wp[r] + k + 512); }
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const bf16x8 x0 = *reinterpret_cast<const bf16x8*>(x + (int64_t)m * ldx + k);
        const bf16x8 x1 = *reinterpret_cast<const bf16x8*>(x + (int64_t)m * ldx + k + 512);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[m][r] = gv_dot8(x1, w1[r], gv_dot8(x0, w0[r], acc[m][r]));
      }
    }
    if (it < iters) {
      bf16x8 w0[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) w0[r] = gv_ldw(wp[r] + k);
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const bf16x8 x0 = *reinterpret_cast<const bf16x8*>(x + (int64_t)m * ldx + k);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[m][r] = gv_dot8(x0, w0[r], acc[m][r]);
      }
    }
    k = iters * 512 + lane * 8;                                // K tail (K % 512 != 0; K % 8 == 0)
    if (k < K) {
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const bf16x8 x0 = *reinterpret_cast<const bf16x8*>(x + (int64_t)m * ldx + k);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[m][r] = gv_dot8(x0, gv_ldw(wp[r] + k), acc[m][r]);
      }
    }
  }

  // four 512-element steps per trip (16 weight loads in flight per lane: one step per trip left every trip waiting on its own 4 loads — the
  // down projection's 21.5 trips per row were 21.5 dependent round trips)
  static __device__ __forceinline__ void row_dot(const bf16_t* __restrict__ xr, const bf16_t* const (&wp)[4], int K, int lane, float (&acc)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = 0.f;
    int k = lane * 8;
    for (; k + 3 * 512 < K; k += 4 * 512) {
      bf16x8 xs[4], ws[4][4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        xs[u] = *reinterpret_cast<const bf16x8*>(xr + k + u * 512);
#pragma unroll
        for (int r = 0; r < 4; ++r) ws[u][r] = gv_ldw(wp[r] + k + u * 512);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = gv_dot8(xs[u], ws[u][r], acc[r]);
    }
    for (; k < K; k += 512) {
      const bf16x8 x0 = *reinterpret_cast<const bf16x8*>(xr + k);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = gv_dot8(x0, gv_ldw(wp[r] + k), acc[r]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = wave_sum(acc[r]);
  }

  // two of the part's 512-element steps per trip (8 weight loads in flight per lane)
  static __device__ __forceinline__ void part_dot(const bf16_t* __restrict__ xr, const bf16_t* const (&wp)[4], int K, int lane, int kp,
                                                  float (&acc)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = 0.f;
    int k = lane * 8 + kp * 512;
    for (; k + 2048 < K; k += 4096) {
      const bf16x8 x0 = *reinterpret_cast<const bf16x8*>(xr + k), x1 = *reinterpret_cast<const bf16x8*>(xr + k + 2048);
      bf16x8 w0[4], w1[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) { w0[r] = gv_ldw(wp[r] + k); w1[r] = gv_ldw(wp[r] + k + 2048); }
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = gv_dot8(x1, w1[r], gv_dot8(x0, w0[r], acc[r]));
    }
    if (k < K) {
      const bf16x8 x0 = *reinterpret_cast<const bf16x8*>(xr + k);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = gv_dot8(x0, gv_ldw(wp[r] + k), acc[r]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = wave_sum(acc[r]);
  }
};

// A 16-byte load carries sixteen codes, so a step of a wave covers 1024 elements of K against 32 bytes of x per lane; a ragged last step
// (K % 1024) has fewer lanes.  All three streams are gq_stream.
struct WeightInt8 {
  using elem = int8_t;
  static constexpr bool SCALED = true;

  template <int M>
  static __device__ __forceinline__ void shared_dot(const bf16_t* __restrict__ x, int64_t ldx, const int8_t* const (&wp)[4], int K, int lane,
                                                    float (&acc)[M][4]) {
    gq_stream<M>(x, ldx, wp, lane * 16, 1024, K, acc);
  }
  static __device__ __forceinline__ void one_row(const bf16_t* __restrict__ xr, const int8_t* const (&wp)[4], int k, int kstep, int K,
                                                 float (&acc)[4]) {
    float part[1][4] = {{0.f, 0.f, 0.f, 0.f}};
    gq_stream<1>(xr, 0, wp, k, kstep, K, part);
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = wave_sum(part[0][r]);
  }
  static __device__ __forceinline__ void row_dot(const bf16_t* __restrict__ xr, const int8_t* const (&wp)[4], int K, int lane, float (&acc)[4]) {
    one_row(xr, wp, lane * 16, 1024, K, acc);
  }
  static __device__ __forceinline__ void part_dot(const bf16_t* __restrict__ xr, const int8_t* const (&wp)[4], int K, int lane, int kp,
                                                  float (&acc)[4]) {
    one_row(xr, wp, lane * 16 + kp * 1024, 4096, K, acc);
  }
};

// ---------------- the three forms ----------------
// SHARED: all M rows use the same W (W rows are loaded once and reused for every x row)
template <class WT, int M, bool SWIGLU>
__global__ __launch_bounds__(256) void gemv_shared_kernel(GemvArgsT<typename WT::elem> g) {
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
  int rows[4];
  gv_wave_rows<SWIGLU>(wid, rows);                          // plain: 4 consecutive columns; SWIGLU: two gate rows and their up rows
  if (rows[0] >= g.N) return;
  const typename WT::elem* wp[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) wp[r] = g.W + (int64_t)min(rows[r], g.N - 1) * g.ldw;
  float acc[M][4];
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[m][r] = 0.f;
  WT::template shared_dot<M>(g.x, g.ldx, wp, g.K, lane, acc);
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[m][r] = wave_sum(acc[m][r]);
  if (lane != 0) return;
  float sc[4];
  if constexpr (WT::SCALED) {
#pragma unroll
    for (int r = 0; r < 4; ++r) sc[r] = g.scale[min(rows[r], g.N - 1)];
  }
#pragma unroll
  for (int m = 0; m < M; ++m) {
    if constexpr (WT::SCALED) {
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[m][r] = sc[r] * acc[m][r];
    }
    if (SWIGLU) {
      gv_swiglu_store(acc[m], rows, g.N, g.alpha, reinterpret_cast<bf16_t*>(g.y) + (int64_t)m * g.ldy);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (rows[r] < g.N) gv_store_shared(g, m, rows[r], acc[m][r]);
    }
  }
}

// INDEXED: every row picks its own weight matrix (and scales): MoE experts; rows are processed one after the other.  A capacity-dropped
// row streams no weights: the plain form stores gv_store_dropped, the SwiGLU form leaves its row unwritten.  DROPS = the launch has a
// row_keep: without one the row loop has no drop test and no branch ahead of the stream (with them, measured on the bf16 gate|up launch of
// four beams, which passes none: 8.52 against 8.42 ms per step; profiles/gemv_forms.md).
template <class WT, bool SWIGLU, bool DROPS>
__global__ __launch_bounds__(256) void gemv_indexed_kernel(GemvArgsT<typename WT::elem> g) {
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
  int rows[4];
  gv_wave_rows<SWIGLU>(wid, rows);
  if (rows[0] >= g.N) return;
  for (int m = 0; m < g.M; ++m) {
    int e;
    if constexpr (DROPS) {
      const GvRow row = gv_row(g, m);
      e = row.e;
      if (row.dropped) {
        if (!SWIGLU && lane < 4 && wid * 4 + lane < g.N) gv_store_dropped(g, m, wid * 4 + lane);
        continue;
      }
    } else {
      e = g.w_index[m];
    }
    const typename WT::elem* Wm = g.W + (int64_t)e * g.strideW;
    const typename WT::elem* wp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) wp[r] = Wm + (int64_t)min(rows[r], g.N - 1) * g.ldw;
    float acc[4];
    WT::row_dot(g.x + (int64_t)m * g.ldx, wp, g.K, lane, acc);
    if (lane != 0) continue;
    if constexpr (WT::SCALED) {
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = g.scale[(int64_t)e * g.strideScale + min(rows[r], g.N - 1)] * acc[r];
    }
    if (SWIGLU) {
      gv_swiglu_store(acc, rows, g.N, 1.f, reinterpret_cast<bf16_t*>(g.y) + (int64_t)m * g.ldy);
    } else {
      const float scale = gv_row_scale(g, m);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (rows[r] < g.N) gv_store_indexed(g, m, rows[r], acc[r], scale);
    }
  }
}

// K-SPLIT form for the narrow projections of a decode step (N <= 4096: o_proj and the down projections, one row of x or the indexed
// expert form).  With a wave per four W rows those launches are 256 workgroups of four waves — one wave per SIMD, 8-16 KB of loads in
// flight per wave and nothing to hide their latency behind: the o projection streamed at 3.2 TB/s, the expert down projection at 4.2
// (gate|up, 1376 workgroups: 5.9).  Here a workgroup of SIXTEEN waves owns the same sixteen W rows: wave (rg, kp) takes the four rows
// of row group rg and every fourth step of K (WT::part_dot), so a CU has four times the loads in flight and four waves per SIMD; the
// four K parts of a row are added in ascending kp order through LDS (a fixed order: deterministic, but not the single-wave order of
// gemv_shared_kernel — the two forms agree to fp32 rounding, not bit for bit).
// Round 5, measured and dropped: the same kernel with EVERY weight load of a row requested before the first multiply (five steps of 4 x 16
// bytes per lane up front, the x row through LDS; a CU's 352 KB share of the down projection fits its register file): 21.4 us against this
// form's 18.8 on the 90 MB down projection, bit-identical.  A launch here is ~4 us of fixed cost (dispatch, first latency, reduction,
// epilogue) + bytes / 6.3 TB/s — qkv 16.0 + 3.3, o 5.3 + 3.9, gate|up 28.6 + 1.9, down 14.3 + 4.5 (profiles/r05a_decode_timeline_dense.md) —
// and the eight loads per lane it keeps in flight already cover the latency; deeper queues only lengthen the register-file fill.
struct KsplitWave {
  int lane, rg, kp, row0, n;       // wave (rg, kp) of the workgroup; rows row0 .. row0 + 3; lane r of the kp = 0 wave finishes row n = row0 + r
  bool fin;
  bool wrote = false;              // red[] holds partials a finishing lane may still be reading
  __device__ __forceinline__ KsplitWave(int N) {
    const int wv = threadIdx.x >> 6;
    lane = threadIdx.x & 63; rg = wv & 3; kp = wv >> 2;
    row0 = (blockIdx.x * 4 + rg) * 4; n = row0 + lane;
    fin = kp == 0 && lane < 4 && n < N;
  }
  // The partial sums acc[r] of this wave's K part -> on a finishing lane, its row's four parts added in ascending kp order.  Called by all
  // sixteen waves (a skipped row is skipped by the whole workgroup).
  __device__ __forceinline__ float sum(float (&red)[4][4][4], const float (&acc)[4]) {     // red: [kp][rg][r]
    if (wrote) __syncthreads();                             // the previous row's partials have been read
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) red[kp][rg][r] = acc[r];
    }
    __syncthreads();
    wrote = true;
    return fin ? ((red[0][rg][lane] + red[1][rg][lane]) + red[2][rg][lane]) + red[3][rg][lane] : 0.f;
  }
};

template <class WT>
__global__ __launch_bounds__(1024) void gemv_ksplit_kernel(GemvArgsT<typename WT::elem> g) {
  __shared__ float red[4][4][4];
  KsplitWave w(g.N);
  for (int m = 0; m < g.M; ++m) {
    const GvRow row = g.w_index ? gv_row(g, m) : GvRow{0, false};
    const int e = row.e;
    if (row.dropped) {                                      // (uniform over the workgroup)
      if (w.fin) gv_store_dropped(g, m, w.n);
      continue;
    }
    const typename WT::elem* Wm = g.W + (int64_t)e * g.strideW;
    const typename WT::elem* wp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) wp[r] = Wm + (int64_t)min(w.row0 + r, g.N - 1) * g.ldw;
    float acc[4];
    WT::part_dot(g.x + (int64_t)m * g.ldx, wp, g.K, w.lane, w.kp, acc);
    float a = w.sum(red, acc);
    if (!w.fin) continue;
    if constexpr (WT::SCALED) a = g.scale[(int64_t)e * g.strideScale + w.n] * a;
    if (g.w_index) gv_store_indexed(g, m, w.n, a, gv_row_scale(g, m));       // gemv_indexed_kernel's epilogue
    else gv_store_shared(g, m, w.n, a);                                        // gemv_shared_kernel's
  }
}

// ---------------- the host dispatch of mp_gemv_bf16 / mp_gemv_w8_bf16 ----------------
template <class WT>
void gemv_launch_shared(const GemvArgsT<typename WT::elem>& g, dim3 grid, hipStream_t s) {      // g.M <= 4
#define MP_GV_SHARED(MM) do { if (g.act == ACT_SWIGLU_PAIR) hipLaunchKernelGGL((gemv_shared_kernel<WT, MM, true>), grid, dim3(256), 0, s, g); \
                              else hipLaunchKernelGGL((gemv_shared_kernel<WT, MM, false>), grid, dim3(256), 0, s, g); } while (0)
  switch (g.M) {
    case 1: MP_GV_SHARED(1); break;
    case 2: MP_GV_SHARED(2); break;
    case 3: MP_GV_SHARED(3); break;
    default: MP_GV_SHARED(4);
  }
#undef MP_GV_SHARED
}

// One launch (5..8 rows of the shared form: two) of the form the shape asks for.  names: what mp_check_launch reports for the shared, the
// indexed and the K-split form of the calling entry point.
template <class WT>
int gemv_launch(const GemvArgsT<typename WT::elem>& g, hipStream_t stream, const char* const (&names)[3]) {
  const int M = g.M, N = g.N, K = g.K, act = g.act;
  const bool w_index = g.w_index != nullptr;
  const int waves = act == ACT_SWIGLU_PAIR ? N / 4 : (int)mp_cdiv(N, 4);
  const dim3 grid((unsigned)mp_cdiv(waves, 4));
  // narrow projections with a long K (o_proj, the down projections of a decode step): sixteen waves per sixteen rows, K split four ways
  if (gv_ksplit_enabled() && act != ACT_SWIGLU_PAIR && N <= 4096 && K >= 4096 && (w_index || M == 1)) {
    hipLaunchKernelGGL(gemv_ksplit_kernel<WT>, grid, dim3(1024), 0, stream, g);
    return mp_check_launch(names[2]);
  }
  if (w_index) {
#define MP_GV_INDEXED(SW) do { if (g.row_keep) hipLaunchKernelGGL((gemv_indexed_kernel<WT, SW, true>), grid, dim3(256), 0, stream, g); \
                               else hipLaunchKernelGGL((gemv_indexed_kernel<WT, SW, false>), grid, dim3(256), 0, stream, g); } while (0)
    if (act == ACT_SWIGLU_PAIR) MP_GV_INDEXED(true);
    else MP_GV_INDEXED(false);
#undef MP_GV_INDEXED
    return mp_check_launch(names[1]);
  }
  if (M <= 4) {
    gemv_launch_shared<WT>(g, grid, stream);
  } else {            // 5..8 rows: two passes of <= 4 over the same weights
    auto a = g; a.M = 4; gemv_launch_shared<WT>(a, grid, stream);
    auto b = g; b.M = M - 4; b.x = g.x + 4 * g.ldx;
    b.y = g.out_f32 ? (void*)(reinterpret_cast<float*>(g.y) + 4 * g.ldy) : (void*)(reinterpret_cast<bf16_t*>(g.y) + 4 * g.ldy);
    if (g.residual) b.residual = g.residual + 4 * g.ldr;
    gemv_launch_shared<WT>(b, grid, stream);
  }
  return mp_check_launch(names[0]);
}

}  // namespace
