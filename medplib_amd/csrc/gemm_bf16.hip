// bf16 MFMA GEMM for gfx950:  C[M,N] = epilogue(A[M,K] · W[N,K]^T)      ("NT": both operands K-contiguous,
// which is nn.Linear's natural layout: activations [tokens, in], weight [out, in]).
//
// Replaces the cuBLAS calls behind every nn.Linear / conv-as-GEMM on the reference hot path
// (HF LlamaAttention/LlamaMLP q,k,v,o,gate,up,down; CLIP fc1/fc2/qkv/out; mm_projector
// model/medplib/model/multimodal_projector/builder.py:39-46; SAM qkv/proj/MLP image_encoder.py:273-296).
//
// Tile: 128x128x64, 256 threads = 4 waves (2x2), each wave 64x64 = 4x4 fragments of
// v_mfma_f32_16x16x32_bf16.  Operands staged global -> VGPR -> LDS (16 B per lane, XOR-swizzled 16-B chunks so the
// ds_read_b128 fragment reads are bank-conflict free), double-buffered LDS, one barrier per K-tile, next tile's
// global loads in flight under the current tile's MFMAs.  XCD-aware block remap keeps one W panel per L2.
#include "common.h"
#include "gemm_common.h"
#include <stdlib.h>
#include <algorithm>

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int NT = 256;

// byte offset of 16-B chunk `c` (0..7) of row `r` in a [rows][64] bf16 LDS tile, XOR-swizzled
__device__ __forceinline__ int lds_off(int r, int c) { return r * 128 + ((c ^ (r & 7)) << 4); }

template <bool GLDS>
__global__ __launch_bounds__(NT, 2) void gemm_bf16_nt_kernel(GemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // [buf][A|W][128*64 bf16 = 16 KiB]
  char* sA0 = smem;
  char* sW0 = smem + 2 * 16384;

  const int batch = blockIdx.y;
  const bf16_t* __restrict__ A = g.A + batch * g.sA;
  const bf16_t* __restrict__ W = g.W + batch * g.sW;
  const int M = g.m_dev ? min(g.M, g.m_dev[batch * g.m_dev_stride]) : g.M;
  const int N = g.N, K = g.K;

  const int tiles_m = (g.M + BM - 1) / BM;
  const int tiles_n = (N + BN - 1) / BN;
  const int nwg = tiles_m * tiles_n;
  // split-K (host-chosen, g.max_split > 1 only for launches with few tiles and a long K, e.g. the SAM adapter convolutions:
  // 24 tiles x 108 K-tiles): unit = split * nwg + tile; partial sums meet in the workspace exactly like the 256x256 kernel's
  // tail split (gemm256_bf16.hip): register-order fp32 partials by agent-scope stores, a ticket per tile, the last arriver sums
  // the S partials in ascending split order and runs the epilogue.
  const int S = g.max_split > 1 ? g.max_split : 1;
  const int split = blockIdx.x / nwg;
  // bijective XCD remap: blocks that land on the same XCD (bid % 8) get a contiguous range of tile ids
  int bid = blockIdx.x - split * nwg;
  const int tile_id = bid;
  {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, loc = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
  }
  // grouped order: ids walk GROUP_M consecutive M-tiles before stepping N, so the ~32-64 workgroups that are co-resident on
  // one XCD cover a GROUP_M x (32/GROUP_M) block of tiles and share both their A and their W panels through that XCD's L2
  const int GROUP_M = g.group_m;
  const int per_group = GROUP_M * tiles_n;
  const int grp = bid / per_group;
  const int first_m = grp * GROUP_M;
  const int gsz = min(tiles_m - first_m, GROUP_M);
  const int tm = first_m + (bid % per_group) % gsz, tn = (bid % per_group) / gsz;
  const int m0 = tm * BM, n0 = tn * BN;
  if (m0 >= M) return;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  int kt0 = 0, nt = K / BK;
  if (S > 1) {
    const int base = nt / S, extra = nt % S;
    kt0 = split * base + min(split, extra);
    nt = base + (split < extra ? 1 : 0);
  }
  const int fr = lane & 15;   // fragment row (A) / col (W) within 16
  const int fq = lane >> 4;   // k-chunk selector 0..3

  auto compute = [&](int buf) {
    const char* sa = sA0 + buf * 16384;
    const char* sw = sW0 + buf * 16384;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = wm * 64 + i * 16 + fr;
        fa[i] = *reinterpret_cast<const bf16x8*>(sa + lds_off(r, kk * 4 + fq));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = wn * 64 + j * 16 + fr;
        fb[j] = *reinterpret_cast<const bf16x8*>(sw + lds_off(r, kk * 4 + fq));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);   // (W, A): transposed accumulators
    }
  };

  if constexpr (GLDS) {
    // Direct global -> LDS DMA (global_load_lds_dwordx4): each wave-instruction fills 1 KiB of LDS lane-linearly, so the
    // XOR swizzle lives on the SOURCE address: LDS chunk position p = instr*64 + lane holds (row p/8, logical chunk
    // (p%8) ^ (row&7)) — the same image lds_off() reads.  Wave w owns instructions w*4 .. w*4+3 of each operand.
    const int sub_row = lane >> 3;                      // 0..7 within the 8-row group of one instruction
    const int src_c = (lane & 7) ^ sub_row;             // logical 16-B chunk this lane fetches
    const bf16_t* a_src[4];
    const bf16_t* w_src[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = (wave * 4 + i) * 8 + sub_row;
      int ar = min(m0 + row, M - 1);
      if (g.a_rows) ar = g.a_rows[batch * g.rows_stride + ar];
      a_src[i] = A + (int64_t)ar * g.lda + src_c * 8 + (int64_t)kt0 * BK;
      w_src[i] = W + (int64_t)min(n0 + row, N - 1) * g.ldw + src_c * 8 + (int64_t)kt0 * BK;
    }
    auto issue = [&](int t, int buf) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int lbase = buf * 16384 + (wave * 4 + i) * 1024;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a_src[i] + (int64_t)t * BK),
                                         (__attribute__((address_space(3))) void*)(sA0 + lbase), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(w_src[i] + (int64_t)t * BK),
                                         (__attribute__((address_space(3))) void*)(sW0 + lbase), 16, 0, 0);
      }
    };
    issue(0, 0);
    for (int t = 0; t < nt; ++t) {
      __syncthreads();                       // tile t landed (vmcnt(0) + barrier); everyone is done reading buf[(t+1)&1]
      if (t + 1 < nt) issue(t + 1, (t + 1) & 1);
      compute(t & 1);
    }
  } else {
    // register-staged variant (global -> VGPR -> ds_write_b128)
    const int ld_row = tid >> 3;   // 0..31  (+32*i)
    const int ld_c = tid & 7;      // 16-B chunk within the 64-wide K slab
    const bf16_t* a_ptr[4];
    const bf16_t* w_ptr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int ar = min(m0 + ld_row + 32 * i, M - 1);
      if (g.a_rows) ar = g.a_rows[batch * g.rows_stride + ar];
      a_ptr[i] = A + (int64_t)ar * g.lda + ld_c * 8 + (int64_t)kt0 * BK;
      w_ptr[i] = W + (int64_t)min(n0 + ld_row + 32 * i, N - 1) * g.ldw + ld_c * 8 + (int64_t)kt0 * BK;
    }
    bf16x8 ra[4], rw[4];
    auto gload = [&](int t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ra[i] = *reinterpret_cast<const bf16x8*>(a_ptr[i] + (int64_t)t * BK);
        rw[i] = *reinterpret_cast<const bf16x8*>(w_ptr[i] + (int64_t)t * BK);
      }
    };
    auto lstore = [&](int buf) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = ld_row + 32 * i;
        *reinterpret_cast<bf16x8*>(sA0 + buf * 16384 + lds_off(r, ld_c)) = ra[i];
        *reinterpret_cast<bf16x8*>(sW0 + buf * 16384 + lds_off(r, ld_c)) = rw[i];
      }
    };
    gload(0);
    lstore(0);
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
      if (t + 1 < nt) gload(t + 1);
      compute(t & 1);
      if (t + 1 < nt) lstore((t & 1) ^ 1);
      __syncthreads();
    }
  }

  if (S > 1) {
    __syncthreads();                                     // all LDS reads of the main loop are done: smem[0] becomes the flag
    unsigned long long* wsu = reinterpret_cast<unsigned long long*>(g.ws) + ((int64_t)(batch * nwg + tile_id) * S) * (BM * BN / 2);
    unsigned long long* mine = wsu + (int64_t)split * (BM * BN / 2);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const unsigned long long v = (unsigned long long)__float_as_uint(acc[i][j][2 * h]) |
                                       ((unsigned long long)__float_as_uint(acc[i][j][2 * h + 1]) << 32);
          __hip_atomic_store(mine + ((i * 4 + j) * 2 + h) * NT + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int* flag = reinterpret_cast<int*>(smem);
    int* ticket_p = g.tickets + batch * nwg + tile_id;
    if (tid == 0) *flag = __hip_atomic_fetch_add(ticket_p, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const int ticket = *flag;
    if (ticket != S - 1) return;
    if (tid == 0) __hip_atomic_store(ticket_p, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int sp = 0; sp < S; ++sp) {
      const unsigned long long* part = wsu + (int64_t)sp * (BM * BN / 2);
      unsigned long long t[32];
#pragma unroll
      for (int q = 0; q < 32; ++q) t[q] = __hip_atomic_load(part + q * NT + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int q = 0; q < 32; ++q) {
        const int i = q >> 3, j = (q >> 1) & 3, h = q & 1;
        acc[i][j][2 * h] += __uint_as_float((unsigned)(t[q] & 0xffffffffull));
        acc[i][j][2 * h + 1] += __uint_as_float((unsigned)(t[q] >> 32));
      }
    }
  }
  // epilogue.  The MFMAs are issued as (W fragment, A fragment), so acc[i][j][r] = C[row = i*16 + fr, col = j*16 + fq*4 + r] of the
  // wave tile: a lane owns four consecutive columns of one row per fragment and stores them as one 8-byte (bf16) / 16-byte (fp32)
  // piece.  Same rounding points as before: activation result rounded to the output type, residual added after.
  if (g.c_rows) {      // combine folded into the epilogue (see gemm256_bf16.hip): out[token] = residual[token] + weight[token] * bf16(acc)
    bf16_t* Co = reinterpret_cast<bf16_t*>(g.C);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = m0 + wm * 64 + i * 16 + fr;
      if (row >= M) continue;
      const int orow = g.c_rows[batch * g.rows_stride + row];
      const float sc = g.c_scale ? g.c_scale[orow] : 1.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = n0 + wn * 64 + j * 16 + fq * 4;
        if (col + 4 > N) continue;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = sc * (float)(bf16_t)acc[i][j][r];
        if (g.residual) {
          const bf16x4 rv = *reinterpret_cast<const bf16x4*>(g.residual + (int64_t)orow * g.ldr + col);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += (float)rv[r];
        }
        *reinterpret_cast<bf16x4*>(Co + (int64_t)orow * g.ldc + col) = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
      }
    }
    return;
  }
  const float* bias = g.bias ? g.bias + batch * g.sBias : nullptr;
  const bf16_t* R = g.residual ? g.residual + batch * g.sR : nullptr;
  bf16_t* Cb = g.out_f32 ? nullptr : reinterpret_cast<bf16_t*>(g.C) + batch * g.sC;
  float* Cf = g.out_f32 ? reinterpret_cast<float*>(g.C) + batch * g.sC : nullptr;
  const bool vec = (g.ldc & 3) == 0 && (!R || (g.ldr & 3) == 0);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = n0 + wn * 64 + j * 16 + fq * 4;
    if (col >= N) continue;
    float bv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[r] = (bias && col + r < N) ? bias[col + r] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = m0 + wm * 64 + i * 16 + fr;
      if (row >= M) continue;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = apply_act(acc[i][j][r] * g.alpha + bv[r], g.act);
      if (vec && col + 4 <= N) {
        if (R) {
          const bf16x4 rv = *reinterpret_cast<const bf16x4*>(R + (int64_t)row * g.ldr + col);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += (float)rv[r];
        }
        if (Cf) *reinterpret_cast<f32x4*>(Cf + (int64_t)row * g.ldc + col) = f32x4{v[0], v[1], v[2], v[3]};
        else *reinterpret_cast<bf16x4*>(Cb + (int64_t)row * g.ldc + col) = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (col + r >= N) continue;
          const float f = v[r] + (R ? (float)R[(int64_t)row * g.ldr + col + r] : 0.f);
          if (Cf) Cf[(int64_t)row * g.ldc + col + r] = f;
          else Cb[(int64_t)row * g.ldc + col + r] = (bf16_t)f;
        }
      }
    }
  }
}

}  // namespace

// split-K factor of a 128x128 launch: only when the tile count leaves most of the machine idle, K is long enough to amortise the
// partial-sum round trip, the row count is known on the host and the scratch is registered
static int split128(const GemmArgs& g, int batch, hipStream_t stream, float** ws, int** tickets) {
  static int enabled = -1;
  if (enabled < 0) { const char* e = getenv("MP_GEMM_MAX_SPLIT"); enabled = (e && atoi(e) == 1) ? 0 : 1; }
  if (!enabled || g.m_dev) return 1;
  int64_t bytes = 0;
  mp_gemm_split_workspace(stream, ws, tickets, &bytes);
  if (!*ws) return 1;
  const int64_t tiles = mp_cdiv(g.M, BM) * mp_cdiv(g.N, BN) * batch;
  const int nt = g.K / BK;
  if (tiles > 128 || nt < 8) return 1;
  int S = (int)std::min<int64_t>(std::min<int64_t>(256 / tiles, nt / 4), 16);
  while (S > 1 && tiles * S * (int64_t)BM * BN * 4 > bytes) --S;
  return S < 2 ? 1 : S;
}

// The 128x128 launch of a call the selection (gemm_dispatch.cpp) left to this kernel.  may_split: the dense mp_gemm_bf16_nt only -- a batched
// launch is one workgroup per tile and batch, with one accumulation order per expert.  The caller checks the launch (under its own name).
void mp_launch_gemm128(const GemmArgs& g0, int batch, bool may_split, hipStream_t stream) {
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)gemm_bf16_nt_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    (void)hipFuncSetAttribute((const void*)gemm_bf16_nt_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    attr_set = true;
  }
  GemmArgs g = g0;
  const int tiles = (int)(mp_cdiv(g.M, BM) * mp_cdiv(g.N, BN));
  int split = 1;
  if (may_split) g.max_split = split = split128(g, batch, stream, &g.ws, &g.tickets);
  const dim3 grid(tiles * split, batch);
  if (mp_gemm_variant() >= 1) hipLaunchKernelGGL(gemm_bf16_nt_kernel<true>, grid, dim3(NT), 65536, stream, g);
  else hipLaunchKernelGGL(gemm_bf16_nt_kernel<false>, grid, dim3(NT), 65536, stream, g);
}
