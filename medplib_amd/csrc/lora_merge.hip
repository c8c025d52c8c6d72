// Device-side LoRA merge (peft merge_and_unload, merge_lora_weights_and_save_hf_model_moe.py:339) into a weight matrix that stays separate from its
// pristine source: Wdst[rows[o], c] = bf16(float(Wsrc[rows[o], c]) + scaling * sum_j b[o, j] * a[j, c]).  One streaming pass: every weight is
// read once and written once, 16 bytes per lane; the fp32 master adapters are read as they are (no bf16 images, no [out, in] fp32 delta).
#include "common.h"

#include <algorithm>

struct LoraMergeDesc {
  const bf16_t* src; bf16_t* dst; const float* a; const float* b; const int64_t* rows;
  int64_t ldsrc, lddst;
  int r, fin, fout;
  float scaling;
};
#define MERGE_ROWS 4
static_assert(sizeof(LoraMergeDesc) == 72, "LoraMergeDesc is packed by medplib_amd/model/llama_lora.py as 72 bytes");

// One wave, one 512-column strip (8 columns per lane), output rows phase, phase + phases, ...  R > 0: the strip of `a` (R x 8 floats per lane)
// stays in registers for the whole walk (dword loads: the masters sit at any 4-byte offset of the optimizer's flat buffer); R == 0: any rank
// up to 64, `a` re-read per row (it stays in L2: r x 2 KiB per strip).  b[o, :] is wave-uniform.  The sum runs j = 0 .. r-1 from zero in fp32:
// a fixed order, no atomics.  src may alias dst: a lane writes what it read.
template <int R>
__device__ __forceinline__ void lora_merge_row(const LoraMergeDesc& g, const float (&av)[R > 0 ? R : 1][8], int o, int64_t ro, const bf16x8 w, int c0) {
  const int r = R > 0 ? R : g.r;
  const float* __restrict__ bo = g.b + (int64_t)o * r;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (R > 0) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const float bj = bo[j];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = fmaf(bj, av[j][k], acc[k]);
    }
  } else {
    for (int j = 0; j < r; ++j) {
      const float bj = bo[j];
      const float* __restrict__ aj = g.a + (int64_t)j * g.fin + c0;
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = fmaf(bj, aj[k], acc[k]);
    }
  }
  bf16x8 out;
#pragma unroll
  for (int k = 0; k < 8; ++k) out[k] = f2bf(fmaf(g.scaling, acc[k], bf2f(w[k])));
  *(bf16x8*)(g.dst + ro * g.lddst + c0) = out;
}

template <int R>
__device__ __forceinline__ void lora_merge_strip(const LoraMergeDesc& g, int strip, int phase, int phases) {
  const int lane = threadIdx.x & 63;
  const int c0 = strip * 512 + lane * 8;
  if (c0 >= g.fin) return;                                   // fin % 8 == 0: a lane holds 8 columns or none
  float av[R > 0 ? R : 1][8];
  if (R > 0) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const float* __restrict__ aj = g.a + (int64_t)j * g.fin + c0;
#pragma unroll
      for (int k = 0; k < 8; ++k) av[j][k] = aj[k];
    }
  }
  int o = phase;
  // MERGE_ROWS rows' weights in flight per wave (the registers of `a` at r = 16 leave room for 2 waves per SIMD: the loads' latency is hidden here, not
  // by occupancy); all of them are read before the first is written, and they are different rows
  for (; o + (MERGE_ROWS - 1) * (int64_t)phases < g.fout; o += MERGE_ROWS * phases) {
    int64_t ro[MERGE_ROWS];
    bf16x8 w[MERGE_ROWS];
#pragma unroll
    for (int u = 0; u < MERGE_ROWS; ++u) ro[u] = g.rows[o + u * phases];
#pragma unroll
    for (int u = 0; u < MERGE_ROWS; ++u) w[u] = *(const bf16x8*)(g.src + ro[u] * g.ldsrc + c0);
#pragma unroll
    for (int u = 0; u < MERGE_ROWS; ++u) lora_merge_row<R>(g, av, o + u * phases, ro[u], w[u], c0);
  }
  for (; o < g.fout; o += phases) {
    const int64_t ro = g.rows[o];
    lora_merge_row<R>(g, av, o, ro, *(const bf16x8*)(g.src + ro * g.ldsrc + c0), c0);
  }
}

// The waves of gridDim.x workgroups share one adapter: with at least as many waves as strips every wave keeps ONE strip and the waves of a strip
// split its rows; with fewer, a wave takes several strips in turn, all rows of each.
__device__ __forceinline__ void lora_merge_body(const LoraMergeDesc& g) {
  if (g.r <= 0 || g.r > 64 || g.fin <= 0 || g.fin % 8 != 0 || g.fout <= 0) return;          // the batched table is not seen by the host
  const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
  const int waves = (int)(gridDim.x * (blockDim.x >> 6));
  const int strips = (g.fin + 511) / 512;
  int s = wave, s_step = waves, phase = 0, phases = 1;
  if (waves >= strips) {
    s = wave % strips;
    s_step = strips;                                         // one turn of the loop below
    phase = wave / strips;
    phases = (waves - s + strips - 1) / strips;              // waves that hold strip s
  }
  for (; s < strips; s += s_step) {
    if (g.r == 8) lora_merge_strip<8>(g, s, phase, phases);
    else if (g.r == 16) lora_merge_strip<16>(g, s, phase, phases);
    else lora_merge_strip<0>(g, s, phase, phases);
    if (waves >= strips) break;
  }
}

__global__ __launch_bounds__(256) void lora_merge_rows_kernel(const LoraMergeDesc g) { lora_merge_body(g); }
__global__ __launch_bounds__(256) void lora_merge_rows_batched_kernel(const LoraMergeDesc* __restrict__ descs) { lora_merge_body(descs[blockIdx.y]); }

extern "C" int mp_lora_merge_rows_bf16(const void* Wsrc, int64_t ldsrc, void* Wdst, int64_t lddst, const float* a, const float* b,
                                       const int64_t* rows, int r, int fin, int fout, float scaling, hipStream_t stream) {
  MP_REQUIRE(r > 0 && r <= 64 && fin > 0 && fin % 8 == 0 && fout >= 0, MP_ERR_SHAPE,
             "mp_lora_merge_rows_bf16: 0 < r <= 64, fin %% 8 == 0, fout >= 0 (got r %d, fin %d, fout %d)", r, fin, fout);
  MP_REQUIRE(ldsrc >= fin && lddst >= fin && ldsrc % 8 == 0 && lddst % 8 == 0, MP_ERR_SHAPE,
             "mp_lora_merge_rows_bf16: ldsrc / lddst must be >= fin and multiples of 8 (got %lld, %lld)", (long long)ldsrc, (long long)lddst);
  if (fout == 0) return MP_OK;
  MP_REQUIRE(Wsrc && Wdst && a && b && rows, MP_ERR_ARG, "mp_lora_merge_rows_bf16: null operand");
  MP_REQUIRE(((uintptr_t)Wsrc & 15) == 0 && ((uintptr_t)Wdst & 15) == 0, MP_ERR_ARG, "mp_lora_merge_rows_bf16: Wsrc and Wdst must be 16-byte aligned");
  // memory-bound: at most 2048 workgroups, the rest by the row walk; a wave gets >= 8 rows where there are that many (its strip of `a` is
  // r x 32 bytes per lane against 32 bytes per row)
  const int64_t strips = mp_cdiv(fin, 512);
  const int64_t blocks = std::min<int64_t>(2048, std::max<int64_t>(1, mp_cdiv(strips * mp_cdiv(fout, 8), 4)));
  const LoraMergeDesc g = {(const bf16_t*)Wsrc, (bf16_t*)Wdst, a, b, rows, ldsrc, lddst, r, fin, fout, scaling};
  hipLaunchKernelGGL(lora_merge_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, g);
  return mp_check_launch("mp_lora_merge_rows_bf16");
}

extern "C" int mp_lora_merge_rows_batched(const void* descs, int n, hipStream_t stream) {
  MP_REQUIRE(n >= 0, MP_ERR_SHAPE, "mp_lora_merge_rows_batched: n >= 0 (got %d)", n);
  if (n == 0) return MP_OK;
  MP_REQUIRE(descs, MP_ERR_ARG, "mp_lora_merge_rows_batched: null descriptor table");
  MP_REQUIRE(n <= 65535, MP_ERR_SHAPE, "mp_lora_merge_rows_batched: at most 65535 adapters per launch (got %d)", n);
  // the shapes live on the device: a fixed share of ~4096 workgroups per adapter, each walking its strips and rows
  const int64_t per = std::min<int64_t>(2048, std::max<int64_t>(1, mp_cdiv(4096, n)));
  hipLaunchKernelGGL(lora_merge_rows_batched_kernel, dim3((unsigned)per, (unsigned)n), dim3(256), 0, stream, (const LoraMergeDesc*)descs);
  return mp_check_launch("mp_lora_merge_rows_batched");
}
