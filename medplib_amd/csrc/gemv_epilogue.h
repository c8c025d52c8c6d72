// The epilogues of the decode-step GEMVs (gemv_forms.h, gemv_bf16.hip): what happens to a finished fp32 dot product `a` of output column n of
// row m.  `Args` is the kernel's argument block (GemvArgsT of either weight type).  The rounding points are those of the 256x256 GEMM
// epilogue, so a decode row and a prefill row round at the same places.
#pragma once
#include "gemm_common.h"

// wave `wid`'s four W rows: plain = four consecutive; SWIGLU = gate rows {g0, g0+1} and their up rows {g0+32, g0+33} of the interleaved gate|up matrix
template <bool SWIGLU>
__device__ __forceinline__ void gv_wave_rows(int wid, int (&rows)[4]) {
  if (SWIGLU) {
    const int pair = wid * 2;                               // output column pair index
    const int blk = pair >> 5, j = pair & 31;
    rows[0] = blk * 64 + j; rows[1] = rows[0] + 1; rows[2] = rows[0] + 32; rows[3] = rows[0] + 33;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) rows[r] = wid * 4 + r;
  }
}

// shared-weight form: act(a * alpha + bias) -> [bf16 rounding] -> + residual
template <class Args>
__device__ __forceinline__ void gv_store_shared(const Args& g, int m, int n, float a) {
  float v = apply_act(a * g.alpha + (g.bias ? g.bias[n] : 0.f), g.act);
  if (g.out_f32) {
    if (g.residual) v += (float)g.residual[(int64_t)m * g.ldr + n];
    reinterpret_cast<float*>(g.y)[(int64_t)m * g.ldy + n] = v;
  } else {
    v = (float)(bf16_t)v;                                    // same rounding points as the 256x256 GEMM epilogue
    if (g.residual) v += (float)g.residual[(int64_t)m * g.ldr + n];
    reinterpret_cast<bf16_t*>(g.y)[(int64_t)m * g.ldy + n] = (bf16_t)v;
  }
}

// indexed (expert) form: combine weight on the bf16-rounded expert output, then the residual
template <class Args>
__device__ __forceinline__ void gv_store_indexed(const Args& g, int m, int n, float a, float scale) {
  float v = scale * (float)(bf16_t)a;
  if (g.residual) v += (float)g.residual[(int64_t)m * g.ldr + n];
  reinterpret_cast<bf16_t*>(g.y)[(int64_t)m * g.ldy + n] = (bf16_t)v;
}

// a capacity-dropped row of the indexed form: what scale 0 leaves of the combine, the residual's own bits (+0 without one).  Stored as such and
// not as 0 * bf16(a) + residual, which is -0 for a negative a without a residual (and NaN for a non-finite a)
template <class Args>
__device__ __forceinline__ void gv_store_dropped(const Args& g, int m, int n) {
  reinterpret_cast<bf16_t*>(g.y)[(int64_t)m * g.ldy + n] = g.residual ? g.residual[(int64_t)m * g.ldr + n] : (bf16_t)0.f;
}

// row m of the indexed form: its weight matrix, and whether the capacity limit dropped it (row_keep[m] < 0).  The two loads are requested
// together, with no branch between them (a null row_keep reads w_index[m] in its place and ignores it), so a row waits one round trip ahead
// of its weight stream, not two.  Both arrays were written by earlier launches and m is uniform, so they are read as constant memory (scalar
// loads in every form).  The empty asm wants both values at one point: without it the compiler moves the w_index load behind the drop
// branch, where only the kept row uses it, and the row waits twice.
struct GvRow { int e; bool dropped; };
template <class Args>
__device__ __forceinline__ GvRow gv_row(const Args& g, int m) {
  typedef const int __attribute__((address_space(4))) * const_int_ptr;
  const int* keep = g.row_keep ? g.row_keep : g.w_index;
  int e = ((const_int_ptr)g.w_index)[m], k = ((const_int_ptr)keep)[m];
  asm volatile("" : "+s"(e), "+s"(k));
  return GvRow{e, g.row_keep && k < 0};
}

// the combine weight of a kept row m in the indexed form: row_scale[m] (1 without)
template <class Args>
__device__ __forceinline__ float gv_row_scale(const Args& g, int m) { return g.row_scale ? g.row_scale[m] : 1.f; }

// SwiGLU pairing (lane 0): gate rows {g0, g0+1} = acc[0..1] and their up rows {g0+32, g0+33} = acc[2..3] -> two output columns of yo
__device__ __forceinline__ void gv_swiglu_store(const float (&acc)[4], const int (&rows)[4], int N, float alpha, bf16_t* __restrict__ yo) {
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float gf = (float)(bf16_t)(acc[p] * alpha), uf = (float)(bf16_t)(acc[2 + p] * alpha);
    const int col = (rows[p] >> 6) * 32 + (rows[p] & 31);
    if (rows[p] < N) yo[col] = (bf16_t)(gf * mp_sigmoid_fast(gf) * uf);
  }
}
