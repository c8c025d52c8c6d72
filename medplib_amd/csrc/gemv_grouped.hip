// The GROUPED expert GEMV of a decode step whose rows are the prompts of a batch (generate_batch): mp_gemv_bf16's indexed form with one weight
// stream per EXPERT instead of one per row.  The indexed kernels of gemv_forms.h take the rows one after the other, each streaming its own
// expert's matrix, so B rows of a top-1 layer read B matrices even when E = 2.  Here a wave sorts the kept rows by expert — lane m holds row
// m's (w_index, row_keep), a ballot per group — and streams its four W rows of an expert ONCE against all of that expert's x rows, in passes
// of at most four rows (the shared form's register budget).  An expert no kept row names streams nothing; a dropped row streams nothing.
// Row for row BIT-IDENTICAL with mp_gemv_bf16 given the same arguments: a lane's share of x[m] . W[n] is summed over the same k in the same
// ascending order (wave form: k = 8 lane + 512 s, WeightBf16::row_dot's; K-split form: k = 8 lane + 512 kp + 2048 s, part_dot's), then
// wave_sum, then the four K parts in ascending kp (KsplitWave::sum), then the same epilogues of gemv_epilogue.h.  Only the number of x rows
// that share a loaded W vector differs.  bf16 weights only: the int8 and NF4 copies keep the indexed form.
#include "gemv_forms.h"

namespace {

struct GroupedArgs {
  GemvArgs g;
  int E;
};

// The rows of a launch as a wave sees them: `todo` = the kept rows still to be computed, `dead` = the rows that stream nothing (row_keep < 0, or
// an expert index outside [0, E): such a row is stored as a dropped one instead of reading past the weight tensor).  Wave-uniform.
struct GroupedRows {
  int ev;                          // lane m < M: w_index[m]
  bool live;                       // lane m: row m is kept
  unsigned long long todo, dead;
  __device__ __forceinline__ GroupedRows(const GroupedArgs& a, int lane) {
    const GemvArgs& g = a.g;
    int kv = 0;
    ev = 0;
    if (lane < g.M) { ev = g.w_index[lane]; kv = g.row_keep ? g.row_keep[lane] : 0; }
    live = lane < g.M && kv >= 0 && ev >= 0 && ev < a.E;
    todo = __ballot(live);
    dead = __ballot(lane < g.M && !live);
  }
  // The next pass: the lowest row still to do and up to three more rows of its expert, ascending -> their count; sel = the rows, four bits each.
  __device__ __forceinline__ int next(int& e, unsigned& sel) {
    const int m0 = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
    e = __builtin_amdgcn_readlane(ev, m0);
    unsigned long long grp = __ballot(live && ev == e) & todo;
    int cnt = 0;
    sel = 0;
    while (grp && cnt < 4) {
      const int m = __ffsll((long long)grp) - 1;
      sel |= (unsigned)m << (4 * cnt);
      ++cnt;
      grp &= grp - 1;
      todo &= ~(1ull << m);
    }
    return cnt;
  }
};

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

template <int NR>
__device__ __forceinline__ void gg_x_rows(const GemvArgs& g, unsigned sel, const bf16_t* (&xp)[NR]) {
#pragma unroll
  for (int j = 0; j < NR; ++j) xp[j] = g.x + (int64_t)((sel >> (4 * j)) & 15u) * g.ldx;
}

// ---------------- the wave-per-four-rows form (gate|up with SwiGLU; a plain projection outside the K-split shape) ----------------
template <int NR, bool SWIGLU>
__device__ __forceinline__ void gg_wave_pass(const GemvArgs& g, unsigned sel, const bf16_t* const (&wp)[4], const int (&rows)[4], int lane) {
  const bf16_t* xp[NR];
  gg_x_rows<NR>(g, sel, xp);
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

template <bool SWIGLU>
__global__ __launch_bounds__(256) void gemv_grouped_kernel(GroupedArgs a) {
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
      case 1: gg_wave_pass<1, SWIGLU>(g, sel, wp, rows, lane); break;
      case 2: gg_wave_pass<2, SWIGLU>(g, sel, wp, rows, lane); break;
      case 3: gg_wave_pass<3, SWIGLU>(g, sel, wp, rows, lane); break;
      default: gg_wave_pass<4, SWIGLU>(g, sel, wp, rows, lane);
    }
  }
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
