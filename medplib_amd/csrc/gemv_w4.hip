// 4-bit-weight GEMV for the single-token decode steps (the reference's load_in_4bit with bnb_4bit_quant_type="nf4": model/builder.py:41-47,
// chat.py:89-98): y[m, n] = epilogue(sum over blocks b of absmax[n, b] * sum_{k in b} bf16(NF4[code[n, k]]) * x[m, k]) for M <= 8 rows of bf16 x
// against NF4 codes, two per byte, with one fp32 absmax per 64 weights of a row (nf4.h; the first level of bitsandbytes' format: its second,
// 8-bit quantisation of the absmax, is not built).  0.5625 bytes per weight against int8's 1 and bf16's 2.
// mp_gemv_w4_bf16 goes through THE host dispatch of gemv_forms.h (gemv_launch<WeightNF4>: one predicate for the K-split form, one 4 + (M - 4)
// split, for all three weight types), with the rows per wave, the K-split reduction (KsplitWave) and the epilogues of the other two.  The
// kernel bodies and the argument block are this file's own, as explicit specialisations of the forms' templates: an NF4 row is two arrays (codes
// and absmax) and a workgroup needs a lookup table in LDS ahead of its early exits, which the policy interface of gemv_forms.h (a row is one
// pointer, nothing is set up first) does not carry.  gemv_forms.h and the bf16 and int8 kernels built from it are untouched.
// The grouped expert form of a batch's rows (mp_gemv_grouped_w4_bf16, one code stream per expert) is at the end of the kernels.
// Measured: profiles/w4_decode.md.
#include "gemv_grouped.h"
#include "nf4.h"

namespace {

struct WeightNF4 { using elem = uint8_t; };                   // the tag gemv_launch dispatches on; the streams are nq_stream below

template <>
struct GemvArgsT<uint8_t> {                                   // the argument block of the NF4 kernels
  const bf16_t* x; int64_t ldx;
  const uint8_t* W; int64_t ldw; int64_t strideW;     // codes [N, K/2] or [E, N, K/2]; strides in BYTES
  const float* absmax; int64_t lda; int64_t strideA;   // [N, K/64] or [E, N, K/64]; strides in floats
  void* y; int64_t ldy;
  const float* bias; const bf16_t* residual; int64_t ldr;     // bias: always null (the names gemv_epilogue.h reads)
  const int* w_index; const float* row_scale; const int* row_keep;
  int M, N, K, act, out_f32;
  float alpha;
};
using Nf4Args = GemvArgsT<uint8_t>;

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

struct Nf4Row { const uint8_t* c; const float* a; };          // one W row: its code bytes and its block absmax
__device__ __forceinline__ Nf4Row nq_row(const Nf4Args& g, int e, int n) {
  return Nf4Row{g.W + (int64_t)e * g.strideW + (int64_t)n * g.ldw, g.absmax + (int64_t)e * g.strideA + (int64_t)n * g.lda};
}

// At 0.56 bytes per weight the HBM stream delivers ~20 weights per clock per CU, so a convert-and-FMA per weight (gq_fma16) cannot keep up.
// Here a BYTE of codes indexes a 256-entry LDS table of packed bf16 pairs {NF4[hi nibble], NF4[lo nibble]} and the pair goes into the bf16 dot
// instruction against the x pair as it lies in memory: per two weights one byte extract, one 4-byte LDS read and, per x row, one dot2.
// The table is one 1 KB copy per workgroup, entry `byte` at dword `byte`.  A wave's byte indices fall on the 32 banks at random and a read is
// serialised 2.4-2.6 times (measured: three fifths of the LDS's active cycles are bank-conflict cycles), which leaves the stream at 4.7 TB/s.
// Measured and dropped: the conflict-free layout, a copy per bank (entry `byte` of copy c at dword 32 * byte + c, 32 KB, lane l reading copy
// l & 31), with workgroups of the wave-per-four-rows forms looping over two groups of sixteen rows to spread the 8192-dword fill.  Bit-identical,
// and slower in every launch of the decode step — qkv 10.25 -> 14.87 us, o 6.26 -> 7.68, gate|up 15.05 -> 17.30, down 9.70 -> 10.77; 2.10 ->
// 2.41 ms per token dense, 2.27 -> 2.56 MoE: the fill and the extra address add per lookup cost more than the conflicts (profiles/w4_decode.md).
// The fill is from immediates (nf4_bf16_bits_dev) and ends in THE barrier of these kernels; every wave reaches it: the exits for waves past N
// and the dropped rows come after it.
__device__ __forceinline__ void nq_fill(uint32_t* t) {
  if (threadIdx.x < 256) t[threadIdx.x] = nf4_bf16_bits_dev(threadIdx.x >> 4) | nf4_bf16_bits_dev(threadIdx.x & 15) << 16;
  __syncthreads();
}

template <int V>                                              // V dwords (8 V codes) of one row, non-temporal like every weight stream
__device__ __forceinline__ void nq_ldw(const uint8_t* p, uint32_t (&w)[V]) {
  if constexpr (V == 4) {
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
  } else {
    const u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
    w[0] = v[0]; w[1] = v[1];
  }
}

template <int W>                                              // the eight x values (four pairs) against code dword q of a load
__device__ __forceinline__ void nq_ldx(const bf16_t* p, uint32_t (&x)[W], int q) {
  const u32x4 v = *reinterpret_cast<const u32x4*>(p);
  x[4 * q] = v[0]; x[4 * q + 1] = v[1]; x[4 * q + 2] = v[2]; x[4 * q + 3] = v[3];
}

// One load of 8 V codes of each of the wave's four W rows against the 8 V x values of each of the M rows.  The lookup is done once per byte
// and the dot once per x row.  A load lies inside one block of 64 (V = 4: half of one, V = 2: a quarter), so its partial sum takes the
// block's absmax ONCE, not once per weight.  Order: ascending k inside the load, loads in ascending k — fixed, so two launches agree.
template <int M, int V>
__device__ __forceinline__ void nq_fma(const uint32_t* __restrict__ tab, const uint32_t (&x)[M][4 * V], const uint32_t (&w)[4][V], const float (&am)[4],
                                       float (&acc)[M][4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float part[M];
#pragma unroll
    for (int m = 0; m < M; ++m) part[m] = 0.f;
#pragma unroll
    for (int q = 0; q < V; ++q)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const bf16x2 pair = __builtin_bit_cast(bf16x2, tab[(w[r][q] >> (8 * b)) & 0xffu]);
#pragma unroll
        for (int m = 0; m < M; ++m) part[m] = __builtin_amdgcn_fdot2_f32_bf16(pair, __builtin_bit_cast(bf16x2, x[m][4 * q + b]), part[m], false);
      }
#pragma unroll
    for (int m = 0; m < M; ++m) acc[m][r] = fmaf(am[r], part[m], acc[m][r]);
  }
}

// The weight stream of one wave over NF4 codes: the steps k, k + kstep, ... < K (k = this lane's first element, a multiple of 8 V) of its
// four rows against M rows of x, gq_stream's shape: the NEXT step's codes, absmax and x are requested before this one is multiplied.
// K % 64 == 0, so a lane's load is either whole or past K.  The absmax stream (12.5 % of the code bytes) is loaded non-temporally too.
template <int M, int V>
__device__ __forceinline__ void nq_stream(const uint32_t* __restrict__ tab, const bf16_t* __restrict__ x, int64_t ldx, const Nf4Row (&wp)[4], int k,
                                          int kstep, int K, float (&acc)[M][4]) {
  if (k >= K) return;
  uint32_t w[4][V];
  float am[4];
  uint32_t xs[M][4 * V];
#pragma unroll
  for (int r = 0; r < 4; ++r) { nq_ldw<V>(wp[r].c + (k >> 1), w[r]); am[r] = __builtin_nontemporal_load(wp[r].a + (k >> 6)); }
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int q = 0; q < V; ++q) nq_ldx(x + (int64_t)m * ldx + k + 8 * q, xs[m], q);
#pragma unroll 1
  for (; k < K; k += kstep) {
    uint32_t wn[4][V];
    float an[4];
    uint32_t xn[M][4 * V];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      an[r] = am[r];
#pragma unroll
      for (int q = 0; q < V; ++q) wn[r][q] = w[r][q];
    }
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int q = 0; q < 4 * V; ++q) xn[m][q] = xs[m][q];
    if (k + kstep < K) {
      const int kn = k + kstep;
#pragma unroll
      for (int r = 0; r < 4; ++r) { nq_ldw<V>(wp[r].c + (kn >> 1), wn[r]); an[r] = __builtin_nontemporal_load(wp[r].a + (kn >> 6)); }
#pragma unroll
      for (int m = 0; m < M; ++m)
#pragma unroll
        for (int q = 0; q < V; ++q) nq_ldx(x + (int64_t)m * ldx + kn + 8 * q, xn[m], q);
    }
    nq_fma<M, V>(tab, xs, w, am, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      am[r] = an[r];
#pragma unroll
      for (int q = 0; q < V; ++q) w[r][q] = wn[r][q];
    }
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int q = 0; q < 4 * V; ++q) xs[m][q] = xn[m][q];
  }
}

// 16-byte loads (32 codes per lane, a wave step of 2048 elements) in the wave-per-four-rows forms with one or two x rows; three and four x
// rows take 8-byte loads, which halves the x registers of a step (4 rows x 32 x values x two steps in flight would be 128 VGPRs of x alone).
// The K-split form takes 8-byte loads too: its step is then 1024 elements and the four K parts of o_proj (K = 4096) have one step each —
// with 16-byte loads two of every four waves would have none.

// SHARED: all M rows use the same W.
template <int M, bool SWIGLU>
__device__ __forceinline__ void nq_shared_body(const Nf4Args& g) {
  __shared__ uint32_t tab[256];
  nq_fill(tab);
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
  int rows[4];
  gv_wave_rows<SWIGLU>(wid, rows);
  if (rows[0] >= g.N) return;                             // (no barrier follows)
  Nf4Row wp[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) wp[r] = nq_row(g, 0, min(rows[r], g.N - 1));
  float acc[M][4];
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[m][r] = 0.f;
  if constexpr (M <= 2) nq_stream<M, 4>(tab, g.x, g.ldx, wp, lane * 32, 2048, g.K, acc);
  else nq_stream<M, 2>(tab, g.x, g.ldx, wp, lane * 16, 1024, g.K, acc);
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[m][r] = wave_sum(acc[m][r]);
  if (lane != 0) return;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    if (SWIGLU) {
      gv_swiglu_store(acc[m], rows, g.N, g.alpha, reinterpret_cast<bf16_t*>(g.y) + (int64_t)m * g.ldy);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (rows[r] < g.N) gv_store_shared(g, m, rows[r], acc[m][r]);
    }
  }
}

// INDEXED: every row picks its own matrix of codes and absmax (MoE experts); rows one after the other; a dropped row streams nothing.
template <bool SWIGLU, bool DROPS>
__device__ __forceinline__ void nq_indexed_body(const Nf4Args& g) {
  __shared__ uint32_t tab[256];
  nq_fill(tab);
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
    Nf4Row wp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) wp[r] = nq_row(g, e, min(rows[r], g.N - 1));
    float acc[1][4] = {{0.f, 0.f, 0.f, 0.f}};
    nq_stream<1, 4>(tab, g.x + (int64_t)m * g.ldx, 0, wp, lane * 32, 2048, g.K, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[0][r] = wave_sum(acc[0][r]);
    if (lane != 0) continue;
    if (SWIGLU) {
      gv_swiglu_store(acc[0], rows, g.N, 1.f, reinterpret_cast<bf16_t*>(g.y) + (int64_t)m * g.ldy);
    } else {
      const float scale = gv_row_scale(g, m);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (rows[r] < g.N) gv_store_indexed(g, m, rows[r], acc[0][r], scale);
    }
  }
}

// K-SPLIT (N <= 4096, K >= 4096; one row of x or the indexed form): sixteen waves per sixteen rows, wave (rg, kp) takes every fourth step of
// 1024 elements; the parts are added in ascending kp order (KsplitWave::sum, whose barriers every wave of the workgroup reaches: a dropped row
// is dropped by all of them).
template <>
__global__ __launch_bounds__(1024) void gemv_ksplit_kernel<WeightNF4>(Nf4Args g) {
  __shared__ uint32_t tab[256];
  __shared__ float red[4][4][4];
  nq_fill(tab);
  KsplitWave w(g.N);
  for (int m = 0; m < g.M; ++m) {
    const GvRow row = g.w_index ? gv_row(g, m) : GvRow{0, false};
    const int e = row.e;
    if (row.dropped) {                                      // (uniform over the workgroup)
      if (w.fin) gv_store_dropped(g, m, w.n);
      continue;
    }
    Nf4Row wp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) wp[r] = nq_row(g, e, min(w.row0 + r, g.N - 1));
    float part[1][4] = {{0.f, 0.f, 0.f, 0.f}};
    nq_stream<1, 2>(tab, g.x + (int64_t)m * g.ldx, 0, wp, w.lane * 16 + w.kp * 1024, 4096, g.K, part);
    float acc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = wave_sum(part[0][r]);
    const float a = w.sum(red, acc);
    if (!w.fin) continue;
    if (g.w_index) gv_store_indexed(g, m, w.n, a, gv_row_scale(g, m));
    else gv_store_shared(g, m, w.n, a);
  }
}

// the forms' kernels for WeightNF4: every instance gemv_launch can ask for, each the body above
#define MP_W4_SHARED(MM, SW) template <> __global__ __launch_bounds__(256) void gemv_shared_kernel<WeightNF4, MM, SW>(Nf4Args g) { nq_shared_body<MM, SW>(g); }
MP_W4_SHARED(1, false) MP_W4_SHARED(2, false) MP_W4_SHARED(3, false) MP_W4_SHARED(4, false)
MP_W4_SHARED(1, true) MP_W4_SHARED(2, true) MP_W4_SHARED(3, true) MP_W4_SHARED(4, true)
#undef MP_W4_SHARED
#define MP_W4_INDEXED(SW, DR) template <> __global__ __launch_bounds__(256) void gemv_indexed_kernel<WeightNF4, SW, DR>(Nf4Args g) { nq_indexed_body<SW, DR>(g); }
MP_W4_INDEXED(false, false) MP_W4_INDEXED(false, true) MP_W4_INDEXED(true, false) MP_W4_INDEXED(true, true)
#undef MP_W4_INDEXED

// ---------------- the GROUPED expert form (mp_gemv_grouped_w4_bf16): the indexed form with one code stream per expert ----------------
// The rows of a batch that name the same expert share its stream (gemv_grouped.hip: the row sorting is GroupedRows).  Row for row the bits of
// the indexed form above: nq_fma sums one LOAD's products before the block's absmax is applied, so the load width is part of the arithmetic
// and stays the indexed form's at every pass size — 16 bytes in the wave form (nq_stream<1, 4>), 8 bytes in the K-split form (nq_stream<1, 2>);
// the shared form's switch to 8-byte loads at three and four rows is not available here.

// nq_stream over the rows of a pass, which are not equally spaced in memory: the same trips and, per (x row, W row), the same operations.
template <int NR, int V>
__device__ __forceinline__ void nq_stream_rows(const uint32_t* __restrict__ tab, const bf16_t* const (&xp)[NR], const Nf4Row (&wp)[4], int k, int kstep,
                                               int K, float (&acc)[NR][4]) {
  if (k >= K) return;
  uint32_t w[4][V];
  float am[4];
  uint32_t xs[NR][4 * V];
#pragma unroll
  for (int r = 0; r < 4; ++r) { nq_ldw<V>(wp[r].c + (k >> 1), w[r]); am[r] = __builtin_nontemporal_load(wp[r].a + (k >> 6)); }
#pragma unroll
  for (int j = 0; j < NR; ++j)
#pragma unroll
    for (int q = 0; q < V; ++q) nq_ldx(xp[j] + k + 8 * q, xs[j], q);
#pragma unroll 1
  for (; k < K; k += kstep) {
    uint32_t wn[4][V];
    float an[4];
    uint32_t xn[NR][4 * V];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      an[r] = am[r];
#pragma unroll
      for (int q = 0; q < V; ++q) wn[r][q] = w[r][q];
    }
#pragma unroll
    for (int j = 0; j < NR; ++j)
#pragma unroll
      for (int q = 0; q < 4 * V; ++q) xn[j][q] = xs[j][q];
    if (k + kstep < K) {
      const int kn = k + kstep;
#pragma unroll
      for (int r = 0; r < 4; ++r) { nq_ldw<V>(wp[r].c + (kn >> 1), wn[r]); an[r] = __builtin_nontemporal_load(wp[r].a + (kn >> 6)); }
#pragma unroll
      for (int j = 0; j < NR; ++j)
#pragma unroll
        for (int q = 0; q < V; ++q) nq_ldx(xp[j] + kn + 8 * q, xn[j], q);
    }
    nq_fma<NR, V>(tab, xs, w, am, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      am[r] = an[r];
#pragma unroll
      for (int q = 0; q < V; ++q) w[r][q] = wn[r][q];
    }
#pragma unroll
    for (int j = 0; j < NR; ++j)
#pragma unroll
      for (int q = 0; q < 4 * V; ++q) xs[j][q] = xn[j][q];
  }
}

using GroupedArgsW4 = GroupedArgsT<uint8_t>;
// Passes of two in both forms: a row of x is 32 VGPRs per step in flight with 16-byte loads.  Wave form 199 / 201 VGPRs (two waves per SIMD; with
// passes of four 256 VGPRs and one wave), K-split form 125 VGPRs (passes of four spilled 152 bytes per lane).  profiles/batch_decode.md.
#define MP_NQ_WAVE_PASSES MP_GG_PASSES_OF_TWO
#define MP_NQ_KSPLIT_PASSES MP_GG_PASSES_OF_TWO

template <int NR, bool SWIGLU>
__device__ __forceinline__ void nq_wave_pass(const uint32_t* tab, const Nf4Args& g, unsigned sel, const Nf4Row (&wp)[4], const int (&rows)[4], int lane) {
  const bf16_t* xp[NR];
  gg_x_rows<NR>(g, sel, xp);
  float acc[NR][4];
#pragma unroll
  for (int j = 0; j < NR; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[j][r] = 0.f;
  nq_stream_rows<NR, 4>(tab, xp, wp, lane * 32, 2048, g.K, acc);
#pragma unroll
  for (int j = 0; j < NR; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[j][r] = wave_sum(acc[j][r]);
  if (lane != 0) return;
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int m = (sel >> (4 * j)) & 15u;
    if (SWIGLU) {
      gv_swiglu_store(acc[j], rows, g.N, 1.f, reinterpret_cast<bf16_t*>(g.y) + (int64_t)m * g.ldy);
    } else {
      const float scale = gv_row_scale(g, m);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (rows[r] < g.N) gv_store_indexed(g, m, rows[r], acc[j][r], scale);
    }
  }
}

template <bool SWIGLU>
__global__ __launch_bounds__(256) void gemv_grouped_w4_kernel(GroupedArgsW4 a) {
  __shared__ uint32_t tab[256];
  nq_fill(tab);
  const Nf4Args& g = a.g;
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
  int rows[4];
  gv_wave_rows<SWIGLU>(wid, rows);
  if (rows[0] >= g.N) return;                             // (no barrier follows)
  GroupedRows gr(a, lane);
  if (!SWIGLU && lane < 4 && wid * 4 + lane < g.N) {        // dropped rows: gv_store_dropped (the SwiGLU form leaves them unwritten)
    for (unsigned long long d = gr.dead; d; d &= d - 1) gv_store_dropped(g, __ffsll((long long)d) - 1, wid * 4 + lane);
  }
  while (gr.todo) {
    int e;
    unsigned sel;
    const int cnt = gr.next(e, sel);
    Nf4Row wp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) wp[r] = nq_row(g, e, min(rows[r], g.N - 1));
#define MP_NQ_PASS(NR, SEL) nq_wave_pass<NR, SWIGLU>(tab, g, SEL, wp, rows, lane)
    MP_NQ_WAVE_PASSES(cnt, sel, MP_NQ_PASS);
#undef MP_NQ_PASS
  }
}

template <int NR>
__device__ __forceinline__ void nq_ksplit_pass(const uint32_t* tab, const Nf4Args& g, unsigned sel, const Nf4Row (&wp)[4], KsplitWave& w,
                                               float (&red)[4][4][4]) {
  const bf16_t* xp[NR];
  gg_x_rows<NR>(g, sel, xp);
  float acc[NR][4];
#pragma unroll
  for (int j = 0; j < NR; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[j][r] = 0.f;
  nq_stream_rows<NR, 2>(tab, xp, wp, w.lane * 16 + w.kp * 1024, 4096, g.K, acc);
#pragma unroll
  for (int j = 0; j < NR; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[j][r] = wave_sum(acc[j][r]);
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int m = (sel >> (4 * j)) & 15u;
    const float s = w.sum(red, acc[j]);                      // (every wave of the workgroup: the passes are uniform over it)
    if (w.fin) gv_store_indexed(g, m, w.n, s, gv_row_scale(g, m));
  }
}

__global__ __launch_bounds__(1024) void gemv_grouped_w4_ksplit_kernel(GroupedArgsW4 a) {
  __shared__ uint32_t tab[256];
  __shared__ float red[4][4][4];
  nq_fill(tab);
  const Nf4Args& g = a.g;
  KsplitWave w(g.N);
  GroupedRows gr(a, w.lane);
  if (w.fin) {
    for (unsigned long long d = gr.dead; d; d &= d - 1) gv_store_dropped(g, __ffsll((long long)d) - 1, w.n);
  }
  while (gr.todo) {
    int e;
    unsigned sel;
    const int cnt = gr.next(e, sel);
    Nf4Row wp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) wp[r] = nq_row(g, e, min(w.row0 + r, g.N - 1));
#define MP_NQ_PASS(NR, SEL) nq_ksplit_pass<NR>(tab, g, SEL, wp, w, red)
    MP_NQ_KSPLIT_PASSES(cnt, sel, MP_NQ_PASS);
#undef MP_NQ_PASS
  }
}

// Block-wise absmax quantiser: one workgroup per row, one wave per block of 64 (lane = k inside the block).  absmax = max |w|,
// inv = absmax > 0 ? 1 / absmax : 0, v = w * inv, code = the number of thresholds strictly below v: every step one fp32 operation in that
// order.  A zero block gets absmax 0 and codes 7 (v = 0 lies above the seven negative thresholds).  The even k is the high nibble.
__global__ __launch_bounds__(256) void quantize_blocks_nf4_kernel(const bf16_t* __restrict__ W, int64_t ldw, int K, uint8_t* __restrict__ codes,
                                                                  int64_t ldc, float* __restrict__ absmax, int64_t lda) {
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const bf16_t* w = W + row * ldw;
  uint8_t* c = codes + row * ldc;
  for (int b = threadIdx.x >> 6; b < K / NF4_BLOCK; b += 4) {
    const float f = (float)w[b * NF4_BLOCK + lane];
    const float am = wave_max(fabsf(f));
    const float inv = am > 0.f ? 1.0f / am : 0.f;
    const uint32_t code = nf4_code(f * inv);
    const uint32_t odd = __shfl_down(code, 1, 64);
    if (lane == 0) absmax[row * lda + b] = am;
    if (!(lane & 1)) c[b * (NF4_BLOCK / 2) + (lane >> 1)] = (uint8_t)(code << 4 | odd);
  }
}

}  // namespace

extern "C" int mp_quantize_blocks_nf4_bf16(const void* W, int64_t ldw, int64_t rows, int K, void* codes, int64_t ldc_bytes, float* absmax,
                                           int64_t lda, hipStream_t stream) {
  MP_REQUIRE(rows > 0 && rows < (int64_t)1 << 31 && K > 0 && K % 64 == 0 && ldw >= K && ldc_bytes >= K / 2 && lda >= K / 64, MP_ERR_SHAPE,
             "mp_quantize_blocks_nf4_bf16: rows > 0, K %% 64 == 0 (one absmax per 64), ldw >= K, ldc_bytes >= K / 2, lda >= K / 64 (rows=%lld K=%d)",
             (long long)rows, K);
  MP_REQUIRE(W && codes && absmax, MP_ERR_ARG, "mp_quantize_blocks_nf4_bf16: null operand");
  hipLaunchKernelGGL(quantize_blocks_nf4_kernel, dim3((unsigned)rows), dim3(256), 0, stream, (const bf16_t*)W, ldw, K, (uint8_t*)codes, ldc_bytes,
                     absmax, lda);
  return mp_check_launch("mp_quantize_blocks_nf4_bf16");
}

extern "C" int mp_gemv_w4_bf16(const void* x, int64_t ldx, const void* codes, int64_t ldw_bytes, int64_t strideW_bytes, const float* absmax,
                               int64_t lda, int64_t strideA, void* y, int64_t ldy, const float* bias, const void* residual, int64_t ldr,
                               const int* w_index, const float* row_scale, const int* row_keep, int M, int N, int K, int act, int out_dtype,
                               float alpha, hipStream_t stream) {
  MP_REQUIRE(M >= 1 && M <= GV_MAXM && N > 0 && K > 0 && K % 64 == 0 && ldx % 8 == 0, MP_ERR_SHAPE,
             "mp_gemv_w4_bf16: 1 <= M <= 8, K %% 64 == 0 (M=%d N=%d K=%d)", M, N, K);
  MP_REQUIRE(ldw_bytes % 16 == 0 && strideW_bytes % 16 == 0 && ldw_bytes >= K / 2, MP_ERR_SHAPE,
             "mp_gemv_w4_bf16: ldw_bytes %% 16 == 0 and >= K / 2, strideW_bytes %% 16 == 0 (ldw_bytes=%lld)", (long long)ldw_bytes);
  MP_REQUIRE(lda >= K / 64, MP_ERR_SHAPE, "mp_gemv_w4_bf16: lda >= K / 64 (lda=%lld K=%d)", (long long)lda, K);
  MP_REQUIRE(out_dtype == MP_BF16 || out_dtype == MP_F32, MP_ERR_DTYPE, "mp_gemv_w4_bf16: bad out dtype");
  MP_REQUIRE(!bias, MP_ERR_ARG, "mp_gemv_w4_bf16: no bias (no decode projection has one)");
  MP_REQUIRE(act == ACT_NONE || act == ACT_SWIGLU_PAIR, MP_ERR_ARG, "mp_gemv_w4_bf16: activation NONE or SWIGLU_PAIR only (%d)", act);
  MP_REQUIRE(act != ACT_SWIGLU_PAIR || (N % 64 == 0 && out_dtype == MP_BF16 && !residual), MP_ERR_ARG,
             "mp_gemv_w4_bf16: SWIGLU_PAIR needs N %% 64 == 0, bf16 output, no residual");
  MP_REQUIRE(!w_index || out_dtype == MP_BF16, MP_ERR_ARG, "mp_gemv_w4_bf16: the indexed (expert) form writes bf16");
  MP_REQUIRE(x && codes && absmax && y, MP_ERR_ARG, "mp_gemv_w4_bf16: null operand");
  const Nf4Args g{(const bf16_t*)x, ldx, (const uint8_t*)codes, ldw_bytes, strideW_bytes, absmax, lda, strideA, y, ldy, nullptr,
                  (const bf16_t*)residual, ldr, w_index, row_scale, row_keep, M, N, K, act, out_dtype == MP_F32, alpha};
  static const char* const names[3] = {"mp_gemv_w4_bf16", "mp_gemv_w4_bf16(indexed)", "mp_gemv_w4_bf16(ksplit)"};
  return gemv_launch<WeightNF4>(g, stream, names);
}

extern "C" int mp_gemv_grouped_w4_bf16(const void* x, int64_t ldx, const void* codes, int64_t ldw_bytes, int64_t strideW_bytes, const float* absmax,
                                       int64_t lda, int64_t strideA, void* y, int64_t ldy, const void* residual, int64_t ldr, const int* w_index,
                                       const float* row_scale, const int* row_keep, int M, int N, int K, int E, int act, hipStream_t stream) {
  MP_REQUIRE(M >= 1 && M <= GV_MAXM && N > 0 && K > 0 && K % 64 == 0 && ldx % 8 == 0 && E >= 1, MP_ERR_SHAPE,
             "mp_gemv_grouped_w4_bf16: 1 <= M <= 8, K %% 64 == 0, E >= 1 (M=%d N=%d K=%d E=%d)", M, N, K, E);
  MP_REQUIRE(ldw_bytes % 16 == 0 && strideW_bytes % 16 == 0 && ldw_bytes >= K / 2, MP_ERR_SHAPE,
             "mp_gemv_grouped_w4_bf16: ldw_bytes %% 16 == 0 and >= K / 2, strideW_bytes %% 16 == 0 (ldw_bytes=%lld)", (long long)ldw_bytes);
  MP_REQUIRE(lda >= K / 64, MP_ERR_SHAPE, "mp_gemv_grouped_w4_bf16: lda >= K / 64 (lda=%lld K=%d)", (long long)lda, K);
  MP_REQUIRE(x && codes && absmax && y && w_index, MP_ERR_ARG,
             "mp_gemv_grouped_w4_bf16: null operand (the grouped form is the indexed one: w_index is required)");
  MP_REQUIRE(act == ACT_NONE || act == ACT_SWIGLU_PAIR, MP_ERR_ARG, "mp_gemv_grouped_w4_bf16: only NONE / SWIGLU_PAIR (activation %d)", act);
  MP_REQUIRE(act != ACT_SWIGLU_PAIR || (N % 64 == 0 && !residual), MP_ERR_ARG,
             "mp_gemv_grouped_w4_bf16: SWIGLU_PAIR needs N %% 64 == 0 and no residual");
  const GroupedArgsW4 a{Nf4Args{(const bf16_t*)x, ldx, (const uint8_t*)codes, ldw_bytes, strideW_bytes, absmax, lda, strideA, y, ldy, nullptr,
                                (const bf16_t*)residual, ldr, w_index, row_scale, row_keep, M, N, K, act, 0, 1.f}, E};
  const int waves = act == ACT_SWIGLU_PAIR ? N / 4 : (int)mp_cdiv(N, 4);
  const dim3 grid((unsigned)mp_cdiv(waves, 4));
  if (gv_ksplit_enabled() && act != ACT_SWIGLU_PAIR && N <= 4096 && K >= 4096) {        // gemv_launch's predicate
    hipLaunchKernelGGL(gemv_grouped_w4_ksplit_kernel, grid, dim3(1024), 0, stream, a);
    return mp_check_launch("mp_gemv_grouped_w4_bf16(ksplit)");
  }
  if (act == ACT_SWIGLU_PAIR) hipLaunchKernelGGL(gemv_grouped_w4_kernel<true>, grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(gemv_grouped_w4_kernel<false>, grid, dim3(256), 0, stream, a);
  return mp_check_launch("mp_gemv_grouped_w4_bf16");
}
