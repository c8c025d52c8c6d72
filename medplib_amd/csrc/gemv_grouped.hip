// The GROUPED expert GEMVs of a decode step whose rows are the prompts of a batch (generate_batch): the indexed form of mp_gemv_bf16 and of
// mp_gemv_w8_bf16 with one weight stream per EXPERT instead of one per row (the NF4 twin, mp_gemv_grouped_w4_bf16, is in gemv_w4.hip beside the
// helpers it needs).  The indexed kernels of gemv_forms.h take the rows one after the other, each streaming its own expert's matrix, so B rows
// of a top-1 layer read B matrices even when E = 2.  Here a wave sorts the kept rows by expert — lane m holds row m's (w_index, row_keep), a
// ballot per group (GroupedRows, gemv_grouped.h) — and streams its four W rows of an expert ONCE against all of that expert's x rows, in passes
// of at most four rows (the shared form's register budget; two in the sixteen-wave int8 form).  An expert no kept row names streams nothing; a
// dropped row streams nothing.
// Row for row BIT-IDENTICAL with the indexed form of the same weight type given the same arguments: a lane's share of x[m] . W[n] is summed
// over the same k in the same ascending order (bf16 wave form: k = 8 lane + 512 s, WeightBf16::row_dot's; K-split form: k = 8 lane + 512 kp +
// 2048 s, part_dot's; int8: gq_stream's one FMA per weight at k = 16 lane + 1024 s, or 16 lane + 1024 kp + 4096 s), then wave_sum, then the
// four K parts in ascending kp (KsplitWave::sum), then the row's scale (int8) and the same epilogues of gemv_epilogue.h.  Only the number of x
// rows that share a loaded W vector differs.  Measured: profiles/batch_decode.md.
// The same rule for the top-2 pair (mp_gemv_grouped_top2_gate_up_bf16 / _down_bf16) against gemv_top2_gate_up_kernel / gemv_top2_down_kernel of
// gemv_bf16.hip: the rows are the 2T (token, choice) entries, and the down kernel combines a token's two expert outputs after the last pass.
#include "gemv_grouped.h"

namespace {

// This lane's share of x[row j] . W[row r] for the NR rows of a pass: the steps k0, k0 + kstep, ... < K in ascending order in every (j, r)
// chain.  PAIRS: two steps per trip (8 weight loads in flight per lane, as WeightBf16::shared_dot and part_dot); without, one step per trip —
// the same products in the same order with half the registers (the sixteen-wave form has 128 VGPRs per lane: three and four rows at two steps
// per trip spilled 132 bytes per lane).
template <int NR, bool PAIRS = true>
__device__ __forceinline__ void gg_dot(const bf16_t* const (&xp)[NR], const bf16_t* const (&wp)[4], int k0, int kstep, int K, float (&acc)[NR][4]) {
#pragma unroll
  for (int j = 0; j < NR; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[j][r] = 0.f;
  int k = k0;
#pragma unroll 1
  for (; PAIRS && k + kstep < K; k += 2 * kstep) {
    bf16x8 w0[4], w1[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { w0[r] = gv_ldw(wp[r] + k); w1[r] = gv_ldw(wp[r] + k + kstep); }
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const bf16x8 x0 = *reinterpret_cast<const bf16x8*>(xp[j] + k), x1 = *reinterpret_cast<const bf16x8*>(xp[j] + k + kstep);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[j][r] = gv_dot8(x1, w1[r], gv_dot8(x0, w0[r], acc[j][r]));
      __builtin_amdgcn_sched_barrier(0);                      // (one x row's conversions at a time)
    }
  }
#pragma unroll 1
  for (; k < K; k += kstep) {                               // (with PAIRS: at most one step is left)
    bf16x8 w0[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) w0[r] = gv_ldw(wp[r] + k);
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const bf16x8 x0 = *reinterpret_cast<const bf16x8*>(xp[j] + k);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[j][r] = gv_dot8(x0, w0[r], acc[j][r]);
      if constexpr (!PAIRS) __builtin_amdgcn_sched_barrier(0);      // (one x row's conversions at a time)
    }
  }
#pragma unroll
  for (int j = 0; j < NR; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[j][r] = wave_sum(acc[j][r]);
}

// ---------------- the wave-per-four-rows form (gate|up with SwiGLU; a plain projection outside the K-split shape) ----------------
// TOP2: the rows are the 2T (token, choice) entries of mp_moe_route_top2's layout; entry m reads x row m % T and writes output row m.
template <int NR, bool SWIGLU, bool TOP2>
__device__ __forceinline__ void gg_wave_pass(const GemvArgs& g, unsigned sel, const bf16_t* const (&wp)[4], const int (&rows)[4], int lane, int T) {
  const bf16_t* xp[NR];
  if constexpr (TOP2) gg_x_rows_top2<NR>(g, sel, T, xp);
  else gg_x_rows<NR>(g, sel, xp);
  float acc[NR][4];
  if constexpr (NR == 1) WeightBf16::row_dot(xp[0], wp, g.K, lane, acc[0]);      // a lone row: the indexed form's own stream
  else gg_dot<NR>(xp, wp, lane * 8, 512, g.K, acc);
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

template <bool SWIGLU, bool TOP2>
__device__ __forceinline__ void gg_wave_rows_by_expert(const GroupedArgs& a, int T) {
  const GemvArgs& g = a.g;
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
  int rows[4];
  gv_wave_rows<SWIGLU>(wid, rows);
  if (rows[0] >= g.N) return;
  GroupedRows gr(a, lane);
  if (!SWIGLU && lane < 4 && wid * 4 + lane < g.N) {        // dropped rows: gv_store_dropped (the SwiGLU form leaves them unwritten)
    for (unsigned long long d = gr.dead; d; d &= d - 1) gv_store_dropped(g, __ffsll((long long)d) - 1, wid * 4 + lane);
  }
  while (gr.todo) {
    int e;
    unsigned sel;
    const int cnt = gr.next(e, sel);
    const bf16_t* Wm = g.W + (int64_t)e * g.strideW;
    const bf16_t* wp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) wp[r] = Wm + (int64_t)min(rows[r], g.N - 1) * g.ldw;
    switch (cnt) {
      case 1: gg_wave_pass<1, SWIGLU, TOP2>(g, sel, wp, rows, lane, T); break;
      case 2: gg_wave_pass<2, SWIGLU, TOP2>(g, sel, wp, rows, lane, T); break;
      case 3: gg_wave_pass<3, SWIGLU, TOP2>(g, sel, wp, rows, lane, T); break;
      default: gg_wave_pass<4, SWIGLU, TOP2>(g, sel, wp, rows, lane, T);
    }
  }
}

template <bool SWIGLU>
__global__ __launch_bounds__(256) void gemv_grouped_kernel(GroupedArgs a) {
  gg_wave_rows_by_expert<SWIGLU, false>(a, 0);
}

// top-2 gate|up: act[e] = SwiGLU(x[e % T] . W[expert[e]]) for the kept entries e < 2T, the bits of gemv_top2_gate_up_kernel (gemv_bf16.hip)
__global__ __launch_bounds__(256) void gemv_grouped_top2_gate_up_kernel(GroupedArgs a, int T) {
  gg_wave_rows_by_expert<true, true>(a, T);
}

// ---------------- the sixteen-wave K-split form (the experts' down projection: N <= 4096, K >= 4096) ----------------
template <int NR>
__device__ __forceinline__ void gg_ksplit_pass(const GemvArgs& g, unsigned sel, const bf16_t* const (&wp)[4], KsplitWave& w, float (&red)[4][4][4]) {
  const bf16_t* xp[NR];
  gg_x_rows<NR>(g, sel, xp);
  float acc[NR][4];
  gg_dot<NR, (NR == 1)>(xp, wp, w.lane * 8 + w.kp * 512, 2048, g.K, acc);
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int m = (sel >> (4 * j)) & 15u;
    const float s = w.sum(red, acc[j]);                      // (every wave of the workgroup: the passes are uniform over it)
    if (w.fin) gv_store_indexed(g, m, w.n, s, gv_row_scale(g, m));
  }
}

__global__ __launch_bounds__(1024) void gemv_grouped_ksplit_kernel(GroupedArgs a) {
  __shared__ float red[4][4][4];
  const GemvArgs& g = a.g;
  KsplitWave w(g.N);
  GroupedRows gr(a, w.lane);
  if (w.fin) {
    for (unsigned long long d = gr.dead; d; d &= d - 1) gv_store_dropped(g, __ffsll((long long)d) - 1, w.n);
  }
  while (gr.todo) {
    int e;
    unsigned sel;
    const int cnt = gr.next(e, sel);
    const bf16_t* Wm = g.W + (int64_t)e * g.strideW;
    const bf16_t* wp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) wp[r] = Wm + (int64_t)min(w.row0 + r, g.N - 1) * g.ldw;
    switch (cnt) {
      case 1: gg_ksplit_pass<1>(g, sel, wp, w, red); break;
      case 2: gg_ksplit_pass<2>(g, sel, wp, w, red); break;
      case 3: gg_ksplit_pass<3>(g, sel, wp, w, red); break;
      default: gg_ksplit_pass<4>(g, sel, wp, w, red);
    }
  }
}

// ---------------- top-2 down + combine: gemv_top2_down_kernel (gemv_bf16.hip) with one weight stream per expert ----------------
// The passes come expert by expert, a token's two choices in different passes, so a finishing lane keeps the bf16-rounded expert output of
// every entry for its column in LDS (out[entry][column of the workgroup]: it reads only what it wrote itself, no barrier) and combines after
// the last pass, per token in choice order: acc = 0, acc = fma(weight[e], out[e], acc) for the kept c = 0, 1, then bf16(residual + acc) —
// the per-entry kernel's two FMAs and rounding.  Every wave builds the same GroupedRows, so every wave reaches every barrier of KsplitWave::sum.
template <int NR>
__device__ __forceinline__ void gg_top2_down_pass(const GemvArgs& g, unsigned sel, const bf16_t* const (&wp)[4], KsplitWave& w, float (&red)[4][4][4],
                                                  float (&out)[2 * GV_MAXM][16]) {
  const bf16_t* xp[NR];
  gg_x_rows<NR>(g, sel, xp);                                 // (the x row of entry e is act row e)
  float acc[NR][4];
  if constexpr (NR == 1) WeightBf16::part_dot(xp[0], wp, g.K, w.lane, w.kp, acc[0]);      // a lone entry: the per-entry kernel's own stream
  else gg_dot<NR, false>(xp, wp, w.lane * 8 + w.kp * 512, 2048, g.K, acc);                 // (one step per trip: the 128-VGPR budget)
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int m = (sel >> (4 * j)) & 15u;
    const float s = w.sum(red, acc[j]);                      // (every wave of the workgroup: the passes are uniform over it)
    if (w.fin) out[m][w.rg * 4 + w.lane] = (float)(bf16_t)s;
  }
}

// Pass width: four entries (one step per trip) fit the sixteen-wave form's 128 VGPRs without scratch, as in gemv_grouped_ksplit_kernel.
#define MP_GG_TOP2_DOWN_PASSES MP_GG_PASSES_OF_FOUR

__global__ __launch_bounds__(1024) void gemv_grouped_top2_down_kernel(GroupedArgs a, int T) {
  __shared__ float red[4][4][4];
  __shared__ float out[2 * GV_MAXM][16];
  const GemvArgs& g = a.g;
  KsplitWave w(g.N);
  GroupedRows gr(a, w.lane);
  const unsigned long long kept = gr.todo;                   // (wave-uniform, the same in every wave)
  while (gr.todo) {
    int e;
    unsigned sel;
    const int cnt = gr.next(e, sel);
    const bf16_t* Wm = g.W + (int64_t)e * g.strideW;
    const bf16_t* wp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) wp[r] = Wm + (int64_t)min(w.row0 + r, g.N - 1) * g.ldw;
#define MP_GG_PASS(NR, SEL) gg_top2_down_pass<NR>(g, SEL, wp, w, red, out)
    MP_GG_TOP2_DOWN_PASSES(cnt, sel, MP_GG_PASS);
#undef MP_GG_PASS
  }
  if (!w.fin) return;                                        // (no barrier follows)
  const int col = w.rg * 4 + w.lane;
  for (int t = 0; t < T; ++t) {
    float acc = 0.f;
    for (int c = 0; c < 2; ++c) {
      const int e = c * T + t;
      if ((kept >> e) & 1) acc = fmaf(g.row_scale[e], out[e][col], acc);
    }
    bf16_t* yo = reinterpret_cast<bf16_t*>(g.y) + (int64_t)t * g.ldy;
    yo[w.n] = g.residual ? (bf16_t)((float)g.residual[(int64_t)t * g.ldr + w.n] + acc) : (bf16_t)acc;
  }
}

// ---------------- int8 codes (the copies of enable_decode_8bit): mp_gemv_w8_bf16's indexed form, one code stream per expert ----------------
// gq_fma16 with the four dwords of a load taken strictly one after the other (FENCED): an empty asm that names the accumulators and the next
// dword of each code row keeps the compiler from converting all sixty-four codes of a step to fp32 ahead of the first FMA, which is what
// costs gq_stream its ~110 VGPRs with one row.  The same FMAs in the same order in every chain.
template <int NR>
__device__ __forceinline__ void gq_fma16_fenced(const X16 (&x)[NR], i32x4 (&w)[4], float (&acc)[NR][4]) {
  static_assert(NR == 2, "the fence names the accumulators of a two-row pass");
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float c[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int b = 0; b < 4; ++b) c[r][b] = (float)(int8_t)(w[r][q] >> (8 * b));
#pragma unroll
    for (int m = 0; m < NR; ++m)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const float xf = (float)(q < 2 ? x[m].a[(q & 1) * 4 + b] : x[m].b[(q & 1) * 4 + b]);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[m][r] = fmaf(c[r][b], xf, acc[m][r]);
      }
    if (q < 3) {
      int n0 = w[0][q + 1], n1 = w[1][q + 1], n2 = w[2][q + 1], n3 = w[3][q + 1];
      asm volatile("" : "+v"(n0), "+v"(n1), "+v"(n2), "+v"(n3), "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[0][2]), "+v"(acc[0][3]),
                   "+v"(acc[1][0]), "+v"(acc[1][1]), "+v"(acc[1][2]), "+v"(acc[1][3]));
      w[0][q + 1] = n0; w[1][q + 1] = n1; w[2][q + 1] = n2; w[3][q + 1] = n3;
    }
  }
}

// gq_stream (gemv_forms.h) over the rows of a pass, which are not equally spaced in memory: the same trips — one step of 4 x 16 bytes per lane
// with the next step requested before this one is multiplied — and in every (x row, W row) chain gq_fma16's one FMA per weight in ascending
// k, so a row's sum has the bits of the indexed form's gq_stream<1> however many rows share the loaded codes.
// XPRE = false (the sixteen-wave form with two rows, 128 VGPRs per lane): only the codes are requested a step ahead, the x rows of a step are
// loaded in the trip that multiplies them, after the next step's codes have been requested — they come from the cache while those are in flight.
// With both a step ahead two rows spilled 72 bytes per lane, and 52 with FENCED alone; with both switches the kernel has 128 VGPRs and no scratch.
template <int NR, bool XPRE = true, bool FENCED = false>
__device__ __forceinline__ void gq_stream_rows(const bf16_t* const (&xp)[NR], const int8_t* const (&wp)[4], int k, int kstep, int K,
                                               float (&acc)[NR][4]) {
  if (k >= K) return;
  i32x4 w[4];
  X16 xs[NR];
#pragma unroll
  for (int r = 0; r < 4; ++r) w[r] = gq_ldw(wp[r] + k);
  if constexpr (XPRE) {
#pragma unroll
    for (int j = 0; j < NR; ++j) xs[j] = gq_ldx(xp[j] + k);
  }
#pragma unroll 1
  for (; k < K; k += kstep) {
    i32x4 wn[4] = {w[0], w[1], w[2], w[3]};
    X16 xn[NR];
    if constexpr (XPRE) {
#pragma unroll
      for (int j = 0; j < NR; ++j) xn[j] = xs[j];
    }
    if (k + kstep < K) {
#pragma unroll
      for (int r = 0; r < 4; ++r) wn[r] = gq_ldw(wp[r] + k + kstep);
      if constexpr (XPRE) {
#pragma unroll
        for (int j = 0; j < NR; ++j) xn[j] = gq_ldx(xp[j] + k + kstep);
      }
    }
    if constexpr (!XPRE) {
#pragma unroll
      for (int j = 0; j < NR; ++j) xs[j] = gq_ldx(xp[j] + k);
    }
    if constexpr (FENCED) gq_fma16_fenced<NR>(xs, w, acc);
    else gq_fma16<NR>(xs, w, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) w[r] = wn[r];
    if constexpr (XPRE) {
#pragma unroll
      for (int j = 0; j < NR; ++j) xs[j] = xn[j];
    }
  }
}

using GroupedArgsW8 = GroupedArgsT<int8_t>;
// Pass widths (profiles/batch_decode.md).  Wave form: four rows, 230 VGPRs and two waves per SIMD.  Passes of two (168 VGPRs, three waves) were
// measured too: the gate|up launch alone at two rows per expert 54.0 against 58.9 us, but the 7B batch step, whose rows split 3 + 1 and 4 + 0
// as well, 5.07 against 4.90 ms at B = 4 and 9.00 against 8.64 at B = 8 — the step decides.  K-split form (1024 threads, 128 VGPRs per lane):
// two rows; four spilled 156 bytes per lane.
#define MP_GQ_WAVE_PASSES MP_GG_PASSES_OF_FOUR
#define MP_GQ_KSPLIT_PASSES MP_GG_PASSES_OF_TWO

// the wave-per-four-rows form: passes of up to GQ_WAVE_ROWS rows
template <int NR, bool SWIGLU>
__device__ __forceinline__ void gq_wave_pass(const GemvArgsT<int8_t>& g, int e, unsigned sel, const int8_t* const (&wp)[4], const int (&rows)[4],
                                             int lane) {
  const bf16_t* xp[NR];
  gg_x_rows<NR>(g, sel, xp);
  float acc[NR][4];
#pragma unroll
  for (int j = 0; j < NR; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[j][r] = 0.f;
  gq_stream_rows<NR>(xp, wp, lane * 16, 1024, g.K, acc);
#pragma unroll
  for (int j = 0; j < NR; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[j][r] = wave_sum(acc[j][r]);
  if (lane != 0) return;
  float sc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) sc[r] = g.scale[(int64_t)e * g.strideScale + min(rows[r], g.N - 1)];
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int m = (sel >> (4 * j)) & 15u;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[j][r] = sc[r] * acc[j][r];
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
__global__ __launch_bounds__(256) void gemv_grouped_w8_kernel(GroupedArgsW8 a) {
  const GemvArgsT<int8_t>& g = a.g;
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
  int rows[4];
  gv_wave_rows<SWIGLU>(wid, rows);
  if (rows[0] >= g.N) return;
  GroupedRows gr(a, lane);
  if (!SWIGLU && lane < 4 && wid * 4 + lane < g.N) {        // dropped rows: gv_store_dropped (the SwiGLU form leaves them unwritten)
    for (unsigned long long d = gr.dead; d; d &= d - 1) gv_store_dropped(g, __ffsll((long long)d) - 1, wid * 4 + lane);
  }
  while (gr.todo) {
    int e;
    unsigned sel;
    const int cnt = gr.next(e, sel);
    const int8_t* Wm = g.W + (int64_t)e * g.strideW;
    const int8_t* wp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) wp[r] = Wm + (int64_t)min(rows[r], g.N - 1) * g.ldw;
#define MP_GQ_PASS(NR, SEL) gq_wave_pass<NR, SWIGLU>(g, e, SEL, wp, rows, lane)
    MP_GQ_WAVE_PASSES(cnt, sel, MP_GQ_PASS);
#undef MP_GQ_PASS
  }
}

// the sixteen-wave K-split form: wave (rg, kp) takes the steps kp, kp + 4, ... of 1024 elements (WeightInt8::part_dot's)
template <int NR>
__device__ __forceinline__ void gq_ksplit_pass(const GemvArgsT<int8_t>& g, int e, unsigned sel, const int8_t* const (&wp)[4], KsplitWave& w,
                                               float (&red)[4][4][4]) {
  const bf16_t* xp[NR];
  gg_x_rows<NR>(g, sel, xp);
  float acc[NR][4];
#pragma unroll
  for (int j = 0; j < NR; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[j][r] = 0.f;
  gq_stream_rows<NR, (NR == 1), (NR > 1)>(xp, wp, w.lane * 16 + w.kp * 1024, 4096, g.K, acc);
#pragma unroll
  for (int j = 0; j < NR; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[j][r] = wave_sum(acc[j][r]);
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int m = (sel >> (4 * j)) & 15u;
    float s = w.sum(red, acc[j]);                            // (every wave of the workgroup: the passes are uniform over it)
    if (!w.fin) continue;
    s = g.scale[(int64_t)e * g.strideScale + w.n] * s;
    gv_store_indexed(g, m, w.n, s, gv_row_scale(g, m));
  }
}

__global__ __launch_bounds__(1024) void gemv_grouped_w8_ksplit_kernel(GroupedArgsW8 a) {
  __shared__ float red[4][4][4];
  const GemvArgsT<int8_t>& g = a.g;
  KsplitWave w(g.N);
  GroupedRows gr(a, w.lane);
  if (w.fin) {
    for (unsigned long long d = gr.dead; d; d &= d - 1) gv_store_dropped(g, __ffsll((long long)d) - 1, w.n);
  }
  while (gr.todo) {
    int e;
    unsigned sel;
    const int cnt = gr.next(e, sel);
    const int8_t* Wm = g.W + (int64_t)e * g.strideW;
    const int8_t* wp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) wp[r] = Wm + (int64_t)min(w.row0 + r, g.N - 1) * g.ldw;
#define MP_GQ_PASS(NR, SEL) gq_ksplit_pass<NR>(g, e, SEL, wp, w, red)
    MP_GQ_KSPLIT_PASSES(cnt, sel, MP_GQ_PASS);
#undef MP_GQ_PASS
  }
}

}  // namespace

extern "C" int mp_gemv_grouped_bf16(const void* x, int64_t ldx, const void* W, int64_t ldw, int64_t strideW, void* y, int64_t ldy,
                                    const void* residual, int64_t ldr, const int* w_index, const float* row_scale, const int* row_keep, int M,
                                    int N, int K, int E, int act, hipStream_t stream) {
  MP_REQUIRE(M >= 1 && M <= GV_MAXM && N > 0 && K > 0 && K % 8 == 0 && ldx % 8 == 0 && ldw % 8 == 0 && strideW % 8 == 0 && E >= 1, MP_ERR_SHAPE,
             "mp_gemv_grouped_bf16: 1 <= M <= 8, K %% 8 == 0, E >= 1 (M=%d N=%d K=%d E=%d)", M, N, K, E);
  MP_REQUIRE(x && W && y && w_index, MP_ERR_ARG, "mp_gemv_grouped_bf16: null operand (the grouped form is the indexed one: w_index is required)");
  MP_REQUIRE(act == ACT_NONE || act == ACT_SWIGLU_PAIR, MP_ERR_ARG, "mp_gemv_grouped_bf16: only NONE / SWIGLU_PAIR (activation %d)", act);
  MP_REQUIRE(act != ACT_SWIGLU_PAIR || (N % 64 == 0 && !residual), MP_ERR_ARG, "mp_gemv_grouped_bf16: SWIGLU_PAIR needs N %% 64 == 0 and no residual");
  GroupedArgs a{GemvArgs{(const bf16_t*)x, ldx, (const bf16_t*)W, ldw, strideW, y, ldy, nullptr, (const bf16_t*)residual, ldr, w_index, row_scale,
                         row_keep, M, N, K, act, 0, 1.f}, E};
  const int waves = act == ACT_SWIGLU_PAIR ? N / 4 : (int)mp_cdiv(N, 4);
  const dim3 grid((unsigned)mp_cdiv(waves, 4));
  // gemv_launch's predicate for the K-split form (the indexed form takes it at every M)
  if (gv_ksplit_enabled() && act != ACT_SWIGLU_PAIR && N <= 4096 && K >= 4096) {
    hipLaunchKernelGGL(gemv_grouped_ksplit_kernel, grid, dim3(1024), 0, stream, a);
    return mp_check_launch("mp_gemv_grouped_bf16(ksplit)");
  }
  if (act == ACT_SWIGLU_PAIR) hipLaunchKernelGGL(gemv_grouped_kernel<true>, grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(gemv_grouped_kernel<false>, grid, dim3(256), 0, stream, a);
  return mp_check_launch("mp_gemv_grouped_bf16");
}

extern "C" int mp_gemv_grouped_w8_bf16(const void* x, int64_t ldx, const void* W, int64_t ldw, int64_t strideW, const float* scale,
                                       int64_t strideScale, void* y, int64_t ldy, const void* residual, int64_t ldr, const int* w_index,
                                       const float* row_scale, const int* row_keep, int M, int N, int K, int E, int act, hipStream_t stream) {
  MP_REQUIRE(M >= 1 && M <= GV_MAXM && N > 0 && K > 0 && K % 16 == 0 && ldx % 8 == 0 && ldw % 16 == 0 && strideW % 16 == 0 && E >= 1, MP_ERR_SHAPE,
             "mp_gemv_grouped_w8_bf16: 1 <= M <= 8, K %% 16 == 0, E >= 1 (M=%d N=%d K=%d E=%d)", M, N, K, E);
  MP_REQUIRE(x && W && scale && y && w_index, MP_ERR_ARG,
             "mp_gemv_grouped_w8_bf16: null operand (the grouped form is the indexed one: w_index is required)");
  MP_REQUIRE(act == ACT_NONE || act == ACT_SWIGLU_PAIR, MP_ERR_ARG, "mp_gemv_grouped_w8_bf16: only NONE / SWIGLU_PAIR (activation %d)", act);
  MP_REQUIRE(act != ACT_SWIGLU_PAIR || (N % 64 == 0 && !residual), MP_ERR_ARG,
             "mp_gemv_grouped_w8_bf16: SWIGLU_PAIR needs N %% 64 == 0 and no residual");
  GroupedArgsW8 a{GemvArgsT<int8_t>{(const bf16_t*)x, ldx, (const int8_t*)W, ldw, strideW, y, ldy, nullptr, (const bf16_t*)residual, ldr, w_index,
                                    row_scale, row_keep, M, N, K, act, 0, 1.f, scale, strideScale}, E};
  const int waves = act == ACT_SWIGLU_PAIR ? N / 4 : (int)mp_cdiv(N, 4);
  const dim3 grid((unsigned)mp_cdiv(waves, 4));
  if (gv_ksplit_enabled() && act != ACT_SWIGLU_PAIR && N <= 4096 && K >= 4096) {        // gemv_launch's predicate
    hipLaunchKernelGGL(gemv_grouped_w8_ksplit_kernel, grid, dim3(1024), 0, stream, a);
    return mp_check_launch("mp_gemv_grouped_w8_bf16(ksplit)");
  }
  if (act == ACT_SWIGLU_PAIR) hipLaunchKernelGGL(gemv_grouped_w8_kernel<true>, grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(gemv_grouped_w8_kernel<false>, grid, dim3(256), 0, stream, a);
  return mp_check_launch("mp_gemv_grouped_w8_bf16");
}

// The top-2 pair over the 2 * tokens entries of mp_moe_route_top2's layout: mp_gemv_top2_gate_up_bf16 / mp_gemv_top2_down_bf16 (gemv_bf16.hip)
// with one weight stream per expert; the same checks, and E (an entry whose expert index lies outside [0, E) is a dropped one).
extern "C" int mp_gemv_grouped_top2_gate_up_bf16(const void* x, int64_t ldx, const void* W, int64_t ldw, int64_t strideW, void* act,
                                                 int64_t ldact, const int* expert, const int* slot, int tokens, int N, int K, int E,
                                                 hipStream_t stream) {
  MP_REQUIRE(tokens >= 1 && tokens <= GV_MAXM && N > 0 && N % 64 == 0 && K > 0 && K % 8 == 0 && ldx % 8 == 0 && ldw % 8 == 0 &&
                 strideW % 8 == 0 && ldact >= N / 2 && E >= 1, MP_ERR_SHAPE,
             "mp_gemv_grouped_top2_gate_up_bf16: 1 <= tokens <= 8, N %% 64 == 0, K %% 8 == 0, ld* %% 8 == 0, ldact >= N / 2, E >= 1 "
             "(tokens=%d N=%d K=%d E=%d)", tokens, N, K, E);
  MP_REQUIRE(x && W && act && expert && slot, MP_ERR_ARG, "mp_gemv_grouped_top2_gate_up_bf16: null operand");
  GroupedArgs a{GemvArgs{(const bf16_t*)x, ldx, (const bf16_t*)W, ldw, strideW, act, ldact, nullptr, nullptr, 0, expert, nullptr, slot,
                         2 * tokens, N, K, ACT_SWIGLU_PAIR, 0, 1.f}, E};
  hipLaunchKernelGGL(gemv_grouped_top2_gate_up_kernel, dim3((unsigned)mp_cdiv(N / 4, 4)), dim3(256), 0, stream, a, tokens);
  return mp_check_launch("mp_gemv_grouped_top2_gate_up_bf16");
}

extern "C" int mp_gemv_grouped_top2_down_bf16(const void* act, int64_t ldact, const void* W, int64_t ldw, int64_t strideW, void* y, int64_t ldy,
                                              const void* residual, int64_t ldr, const int* expert, const int* slot, const float* weight,
                                              int tokens, int N, int K, int E, hipStream_t stream) {
  MP_REQUIRE(tokens >= 1 && tokens <= GV_MAXM && N > 0 && K > 0 && K % 8 == 0 && ldact % 8 == 0 && ldw % 8 == 0 && strideW % 8 == 0 &&
                 ldy >= N && (!residual || ldr >= N) && E >= 1, MP_ERR_SHAPE,
             "mp_gemv_grouped_top2_down_bf16: 1 <= tokens <= 8, K %% 8 == 0, ld* %% 8 == 0, ldy >= N, ldr >= N, E >= 1 (tokens=%d N=%d K=%d E=%d)",
             tokens, N, K, E);
  MP_REQUIRE(act && W && y && expert && slot && weight, MP_ERR_ARG, "mp_gemv_grouped_top2_down_bf16: null operand");
  GroupedArgs a{GemvArgs{(const bf16_t*)act, ldact, (const bf16_t*)W, ldw, strideW, y, ldy, nullptr, (const bf16_t*)residual, ldr, expert, weight,
                         slot, 2 * tokens, N, K, ACT_NONE, 0, 1.f}, E};
  hipLaunchKernelGGL(gemv_grouped_top2_down_kernel, dim3((unsigned)mp_cdiv(mp_cdiv(N, 4), 4)), dim3(1024), 0, stream, a, tokens);
  return mp_check_launch("mp_gemv_grouped_top2_down_bf16");
}
