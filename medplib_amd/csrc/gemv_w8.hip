// 8-bit-weight GEMV for the single-token decode steps (the reference worker's --load-8bit: model/serve/model_worker.py:72,100,642 ->
// builder.py:39, bitsandbytes Linear8bitLt): y[m, n] = epilogue(scale[n] * sum_k code[n, k] * x[m, k]) for M <= 8 rows of bf16 x against int8
// codes with one fp32 scale per output row (row-wise absmax, bitsandbytes' weight format; the activations stay bf16: W8A16).  A decode step
// is a weight stream, so halving the bytes of W is what this buys.  The structure is gemv_bf16.hip's, arrived at by measurement there: a
// wave owns four consecutive output rows and streams them with 16-byte non-temporal loads, the next step's four requested before the current
// four are multiplied (gq_stream: why one step per trip and not two); the narrow projections with a long K take the sixteen-wave K-split
// form.  A 16-byte load now carries sixteen weights, so a step of a wave covers 1024 elements of K against 32 bytes of x per lane.  The
// epilogues are gemv_bf16.hip's own (gemv_epilogue.h).  Measured: profiles/w8_decode.md.
#include "gemv_epilogue.h"

namespace {

constexpr int GQ_MAXM = 8;
typedef __attribute__((ext_vector_type(4))) int i32x4;

struct GemvW8Args {
  const bf16_t* x; int64_t ldx;
  const int8_t* W; int64_t ldw; int64_t strideW;     // codes [N, K] or [E, N, K]
  const float* scale; int64_t strideScale;           // [N] or [E, N]
  void* y; int64_t ldy;
  const float* bias; const bf16_t* residual; int64_t ldr;      // (bias: always null, the epilogue's field)
  const int* w_index; const float* row_scale; const int* row_keep;
  int M, N, K, act, out_f32;
  float alpha;
};

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

// The weight stream of one wave: the steps k, k + kstep, ... < K of its four code rows against M rows of x (x + m * ldx), one step of 4 x 16
// bytes per lane per trip with the NEXT step requested before this one is multiplied, so four to eight weight loads per lane are in flight
// all the way.  A trip is one step, not gemv_bf16.hip's two: the compiler converts a trip's codes to fp32 up front whatever the source order
// (scheduling barriers do not hold it back), and two steps' worth is 128 floats: 232 VGPRs in the one-row kernel and spills in the
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

// SHARED: all M rows use the same W (the codes are loaded once and reused for every x row)
template <int M, bool SWIGLU>
__global__ __launch_bounds__(256) void gemv_w8_shared_kernel(GemvW8Args g) {
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
  int rows[4];
  gv_wave_rows<SWIGLU>(wid, rows);
  if (rows[0] >= g.N) return;
  const int8_t* wp[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) wp[r] = g.W + (int64_t)min(rows[r], g.N - 1) * g.ldw;
  float acc[M][4];
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[m][r] = 0.f;
  gq_stream<M>(g.x, g.ldx, wp, lane * 16, 1024, g.K, acc);   // 64 lanes x 16 codes per step; a ragged last step (K % 1024) has fewer lanes
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[m][r] = wave_sum(acc[m][r]);
  if (lane != 0) return;
  float sc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) sc[r] = g.scale[min(rows[r], g.N - 1)];
#pragma unroll
  for (int m = 0; m < M; ++m) {
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[m][r] = sc[r] * acc[m][r];
    if (SWIGLU) {
      gv_swiglu_store(acc[m], rows, g.N, g.alpha, reinterpret_cast<bf16_t*>(g.y) + (int64_t)m * g.ldy);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (rows[r] < g.N) gv_store_shared(g, m, rows[r], acc[m][r]);
    }
  }
}

// INDEXED: every row picks its own expert's codes and scales; rows are processed one after the other.  A capacity-dropped row
// (row_keep[m] < 0) streams no weights: the plain form writes its residual (or 0), the SwiGLU form leaves its row unwritten.
template <bool SWIGLU>
__global__ __launch_bounds__(256) void gemv_w8_indexed_kernel(GemvW8Args g) {
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
  int rows[4];
  gv_wave_rows<SWIGLU>(wid, rows);
  if (rows[0] >= g.N) return;
  for (int m = 0; m < g.M; ++m) {
    if (g.row_keep && g.row_keep[m] < 0) {
      if (!SWIGLU && lane < 4 && wid * 4 + lane < g.N) gv_store_dropped(g, m, wid * 4 + lane);
      continue;
    }
    const int e = g.w_index[m];
    const int8_t* Wm = g.W + (int64_t)e * g.strideW;
    const int8_t* wp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) wp[r] = Wm + (int64_t)min(rows[r], g.N - 1) * g.ldw;
    float part[1][4] = {{0.f, 0.f, 0.f, 0.f}}, acc[4];
    gq_stream<1>(g.x + (int64_t)m * g.ldx, 0, wp, lane * 16, 1024, g.K, part);
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = wave_sum(part[0][r]);
    if (lane != 0) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = g.scale[(int64_t)e * g.strideScale + min(rows[r], g.N - 1)] * acc[r];
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

// K-SPLIT form (N <= 4096, K >= 4096, one row or the indexed form: o_proj and the down projections), gemv_ksplit_kernel's layout: a
// workgroup of sixteen waves owns sixteen rows, wave (rg, kp) takes row group rg and every fourth step of K; the four parts of a row are
// added in ascending kp order through LDS, so a launch is bit-reproducible.  A capacity-dropped row streams no weights.
__global__ __launch_bounds__(1024) void gemv_w8_ksplit_kernel(GemvW8Args g) {
  __shared__ float red[4][4][4];                            // [kp][rg][r]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int rg = wv & 3, kp = wv >> 2;
  const int row0 = (blockIdx.x * 4 + rg) * 4;
  const bool fin = kp == 0 && lane < 4 && row0 + lane < g.N;  // lane r of the kp = 0 wave finishes row r of its group
  const int n = row0 + lane;
  bool wrote = false;                                       // red[] holds partials a finishing lane may still be reading
  for (int m = 0; m < g.M; ++m) {
    const int e = g.w_index ? g.w_index[m] : 0;
    if (g.w_index && g.row_keep && g.row_keep[m] < 0) {     // (uniform over the workgroup)
      if (fin) gv_store_dropped(g, m, n);
      continue;
    }
    const int8_t* Wm = g.W + (int64_t)e * g.strideW;
    const int8_t* wp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) wp[r] = Wm + (int64_t)min(row0 + r, g.N - 1) * g.ldw;
    float part[1][4] = {{0.f, 0.f, 0.f, 0.f}}, acc[4];
    gq_stream<1>(g.x + (int64_t)m * g.ldx, 0, wp, lane * 16 + kp * 1024, 4096, g.K, part);      // K part kp: the steps kp, kp + 4, ...
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = wave_sum(part[0][r]);
    if (wrote) __syncthreads();                             // the previous row's partials have been read
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) red[kp][rg][r] = acc[r];
    }
    __syncthreads();
    wrote = true;
    if (!fin) continue;
    const float a = g.scale[(int64_t)e * g.strideScale + n] * (((red[0][rg][lane] + red[1][rg][lane]) + red[2][rg][lane]) + red[3][rg][lane]);
    if (g.w_index) gv_store_indexed(g, m, n, a, gv_row_scale(g, m));
    else gv_store_shared(g, m, n, a);
  }
}

// Row-wise absmax quantiser: one workgroup per row.  scale = absmax / 127, code = rint(w * (127 / absmax)) (half to even), every step one
// fp32 operation in that order; a zero row gets scale 0 and codes 0.
__global__ __launch_bounds__(256) void quantize_rows_w8_kernel(const bf16_t* __restrict__ W, int64_t ldw, int K, int8_t* __restrict__ codes,
                                                               int64_t ldc, float* __restrict__ scale) {
  __shared__ float red[16];
  const int64_t row = blockIdx.x;
  const bf16_t* w = W + row * ldw;
  float mx = 0.f;
  for (int k = threadIdx.x; k < K; k += 256) mx = fmaxf(mx, fabsf((float)w[k]));
  const float absmax = block_max(mx, red);
  if (threadIdx.x == 0) scale[row] = absmax / 127.f;
  const float inv = absmax > 0.f ? 127.f / absmax : 0.f;
  int8_t* c = codes + row * ldc;
  for (int k = threadIdx.x; k < K; k += 256) c[k] = (int8_t)(int)rintf((float)w[k] * inv);
}

template <int M>
void launch_w8_shared(const GemvW8Args& g, dim3 grid, hipStream_t s) {
  if (g.act == ACT_SWIGLU_PAIR) hipLaunchKernelGGL((gemv_w8_shared_kernel<M, true>), grid, dim3(256), 0, s, g);
  else hipLaunchKernelGGL((gemv_w8_shared_kernel<M, false>), grid, dim3(256), 0, s, g);
}

void launch_w8_shared_m(const GemvW8Args& g, dim3 grid, hipStream_t s) {
  switch (g.M) {
    case 1: launch_w8_shared<1>(g, grid, s); break;
    case 2: launch_w8_shared<2>(g, grid, s); break;
    case 3: launch_w8_shared<3>(g, grid, s); break;
    default: launch_w8_shared<4>(g, grid, s);
  }
}

}  // namespace

extern "C" int mp_quantize_rows_w8_bf16(const void* W, int64_t ldw, int64_t rows, int K, void* codes, int64_t ldc, float* scale,
                                        hipStream_t stream) {
  MP_REQUIRE(rows > 0 && rows < (int64_t)1 << 31 && K > 0 && K % 16 == 0 && ldw >= K && ldc >= K, MP_ERR_SHAPE,
             "mp_quantize_rows_w8_bf16: rows > 0, K %% 16 == 0 (what mp_gemv_w8_bf16 reads), ldw >= K, ldc >= K (rows=%lld K=%d)", (long long)rows, K);
  MP_REQUIRE(W && codes && scale, MP_ERR_ARG, "mp_quantize_rows_w8_bf16: null operand");
  hipLaunchKernelGGL(quantize_rows_w8_kernel, dim3((unsigned)rows), dim3(256), 0, stream, (const bf16_t*)W, ldw, K, (int8_t*)codes, ldc, scale);
  return mp_check_launch("mp_quantize_rows_w8_bf16");
}

extern "C" int mp_gemv_w8_bf16(const void* x, int64_t ldx, const void* W, int64_t ldw, int64_t strideW, const float* scale, int64_t strideScale,
                               void* y, int64_t ldy, const float* bias, const void* residual, int64_t ldr, const int* w_index,
                               const float* row_scale, const int* row_keep, int M, int N, int K, int act, int out_dtype, float alpha,
                               hipStream_t stream) {
  MP_REQUIRE(M >= 1 && M <= GQ_MAXM && N > 0 && K > 0 && K % 16 == 0 && ldx % 8 == 0 && ldw % 16 == 0 && strideW % 16 == 0, MP_ERR_SHAPE,
             "mp_gemv_w8_bf16: 1 <= M <= 8, K %% 16 == 0 (M=%d N=%d K=%d)", M, N, K);
  MP_REQUIRE(out_dtype == MP_BF16 || out_dtype == MP_F32, MP_ERR_DTYPE, "mp_gemv_w8_bf16: bad out dtype");
  MP_REQUIRE(!bias, MP_ERR_ARG, "mp_gemv_w8_bf16: no bias (no decode projection has one)");
  MP_REQUIRE(act == ACT_NONE || act == ACT_SWIGLU_PAIR, MP_ERR_ARG, "mp_gemv_w8_bf16: activation NONE or SWIGLU_PAIR only (%d)", act);
  MP_REQUIRE(act != ACT_SWIGLU_PAIR || (N % 64 == 0 && out_dtype == MP_BF16 && !residual), MP_ERR_ARG,
             "mp_gemv_w8_bf16: SWIGLU_PAIR needs N %% 64 == 0, bf16 output, no residual");
  MP_REQUIRE(!w_index || out_dtype == MP_BF16, MP_ERR_ARG, "mp_gemv_w8_bf16: the indexed (expert) form writes bf16");
  MP_REQUIRE(x && W && scale && y, MP_ERR_ARG, "mp_gemv_w8_bf16: null operand");
  GemvW8Args g{(const bf16_t*)x, ldx, (const int8_t*)W, ldw, strideW, scale, strideScale, y, ldy, nullptr, (const bf16_t*)residual, ldr,
               w_index, row_scale, row_keep, M, N, K, act, out_dtype == MP_F32, alpha};
  const int waves = act == ACT_SWIGLU_PAIR ? N / 4 : (int)mp_cdiv(N, 4);
  const dim3 grid((unsigned)mp_cdiv(waves, 4));
  if (act != ACT_SWIGLU_PAIR && N <= 4096 && K >= 4096 && (w_index || M == 1)) {      // mp_gemv_bf16's condition for its K-split form
    hipLaunchKernelGGL(gemv_w8_ksplit_kernel, grid, dim3(1024), 0, stream, g);
    return mp_check_launch("mp_gemv_w8_bf16(ksplit)");
  }
  if (w_index) {
    if (act == ACT_SWIGLU_PAIR) hipLaunchKernelGGL(gemv_w8_indexed_kernel<true>, grid, dim3(256), 0, stream, g);
    else hipLaunchKernelGGL(gemv_w8_indexed_kernel<false>, grid, dim3(256), 0, stream, g);
    return mp_check_launch("mp_gemv_w8_bf16(indexed)");
  }
  if (M <= 4) {
    launch_w8_shared_m(g, grid, stream);
  } else {            // 5..8 rows: two passes of <= 4 over the same codes
    GemvW8Args a = g; a.M = 4; launch_w8_shared_m(a, grid, stream);
    GemvW8Args b = g; b.M = M - 4; b.x = g.x + 4 * ldx;
    b.y = g.out_f32 ? (void*)(reinterpret_cast<float*>(y) + 4 * ldy) : (void*)(reinterpret_cast<bf16_t*>(y) + 4 * ldy);
    if (g.residual) b.residual = g.residual + 4 * ldr;
    launch_w8_shared_m(b, grid, stream);
  }
  return mp_check_launch("mp_gemv_w8_bf16");
}
