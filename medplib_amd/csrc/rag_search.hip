// Image retrieval of in-context examples (model/rag/image_rag.py): the exact fp32 inner-product top-k over an embedding index, and the
// pooled, normalised CLIP embedding that fills it.
//
//   mp_dot_topk_f32          scores[q, :k], idx[q, :k] = top-k over n of <index[n], query[q]>, exact fp32 (f32 in, f32 accumulate),
//                            descending score, ties to the lower index; k > N fills the tail with (-inf, -1).
//     Q == 1   streaming GEMV: every wave holds 4 index rows in flight (float4 per lane, 1 KB per row per load), reduces each
//              row across the wave and keeps its running top-k spread over its lanes (lane p = entry p).  A pure HBM stream.
//     Q >  1   v_mfma_f32_32x32x2_f32 tiles of 128 candidates x 128 queries per workgroup (4 waves, 2 x 2 32x32 tiles each), operands
//              straight from global memory one 32-k chunk ahead; after each candidate tile the 128 x 128 scores go to LDS and one
//              thread per query folds them into its running list.  The [Q, N] score matrix never leaves the CU.
//     Both write one sorted partial list per (query, part) to the workspace; dot_topk_merge_kernel merges the parts of a query.
//   mp_clip_pool_normalize_bf16   m = bf16(mean over rows 1..S-1 of the last hidden state, fp32 sum), out = m / (||m||_2 + 1e-12)
//   mp_l2_normalize_rows_f32      out = x / (||x||_2 + 1e-12) per row (the second normalisation of load_index)
//
// Ranking key: an entry is the 64-bit unsigned key (orderable(score) << 32) | ~idx, so "better" is one integer compare: higher score,
// then lower index.  -0.0 is ranked as +0.0 (float equality), and the key 0 is the empty entry.
#include "common.h"
#include <math.h>
#include <algorithm>

namespace {

constexpr int TK_MAX = 64;
constexpr int MM_TILE = 128;          // candidates x queries per workgroup tile of the batched kernel
constexpr int GEMV_ROWS = 4;          // index rows in flight per wave (Q == 1)
constexpr int GEMV_MAX_BLOCKS = 1024;
constexpr int MM_TARGET_BLOCKS = 256; // one 128 KB-LDS workgroup per CU
constexpr int MERGE_THREADS = 256;
constexpr int MM_BLOCK_CHUNKS = 4;    // the batched kernel sums k in blocks of 4 x 32 (fresh MFMA chain each), then adds the blocks

__device__ __forceinline__ uint64_t topk_key(float s, int idx) {
  if (s == 0.f) s = 0.f;                                         // -0 ranks as +0
  uint32_t u = __float_as_uint(s);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((uint64_t)u << 32) | (uint32_t)(~(uint32_t)idx);
}

__device__ __forceinline__ void topk_unkey(uint64_t key, float* s, int* idx) {
  if (key == 0) {
    *s = -INFINITY;
    *idx = -1;
    return;
  }
  uint32_t u = (uint32_t)(key >> 32);
  u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  *s = __uint_as_float(u);
  *idx = (int)(~(uint32_t)key);
}

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
  return ((uint64_t)hi << 32) | lo;
}

// A wave's sorted list, lane p holding entry p (p < k; lanes >= k hold whatever shifts into them).  Keys are distinct, so the
// insertion point is the number of entries above the new key.
__device__ __forceinline__ uint64_t wave_list_insert(uint64_t mine, uint64_t key, int lane) {
  const int pos = __popcll(__ballot(mine > key));
  const uint64_t up = shfl_u64(mine, lane > 0 ? lane - 1 : 0);
  return lane < pos ? mine : (lane == pos ? key : up);
}

// ---------------------------------------------------------------------------------------------------------------- Q == 1: GEMV
__global__ __launch_bounds__(256) void dot_topk_gemv_kernel(const float* __restrict__ index, int64_t ld, const float* __restrict__ q,
                                                            int N, int C, int k, int rows_per_block, uint64_t* __restrict__ parts) {
  __shared__ uint64_t lists[4][TK_MAX];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r_begin = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r_end = min((int64_t)N, r_begin + rows_per_block);
  uint64_t mine = 0, thr = 0;
  for (int64_t r0 = r_begin + (int64_t)w * GEMV_ROWS; r0 < r_end; r0 += 4 * GEMV_ROWS) {
    float acc[GEMV_ROWS];
    const float* rp[GEMV_ROWS];
#pragma unroll
    for (int j = 0; j < GEMV_ROWS; ++j) {
      acc[j] = 0.f;
      rp[j] = index + min(r0 + j, r_end - 1) * ld;               // rows past the end re-read the last one and are not ranked
    }
#pragma unroll 2
    for (int c = 4 * lane; c < C; c += 256) {
      const float4 qv = *reinterpret_cast<const float4*>(q + c);
      float4 xv[GEMV_ROWS];
#pragma unroll
      for (int j = 0; j < GEMV_ROWS; ++j) {
        const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(rp[j] + c));    // streamed once: keep it out of L2
        xv[j] = make_float4(v[0], v[1], v[2], v[3]);
      }
#pragma unroll
      for (int j = 0; j < GEMV_ROWS; ++j) {
        acc[j] = fmaf(xv[j].x, qv.x, acc[j]);
        acc[j] = fmaf(xv[j].y, qv.y, acc[j]);
        acc[j] = fmaf(xv[j].z, qv.z, acc[j]);
        acc[j] = fmaf(xv[j].w, qv.w, acc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < GEMV_ROWS; ++j) {
      const float s = wave_sum(acc[j]);
      if (r0 + j < r_end) {
        const uint64_t key = topk_key(s, (int)(r0 + j));
        if (key > thr) {
          mine = wave_list_insert(mine, key, lane);
          thr = shfl_u64(mine, k - 1);
        }
      }
    }
  }
  // the block's four wave lists -> one: wave 0 inserts the other three
  if (lane < k) lists[w][lane] = mine;
  __syncthreads();
  if (w == 0) {
    for (int v = 1; v < 4; ++v)
      for (int p = 0; p < k; ++p) {
        const uint64_t key = lists[v][p];
        if (key <= thr) break;                                   // the rest of that sorted list ranks lower still
        mine = wave_list_insert(mine, key, lane);
        thr = shfl_u64(mine, k - 1);
      }
    if (lane < k) parts[(int64_t)blockIdx.x * k + lane] = mine;
  }
}

// ---------------------------------------------------------------------------------------------------------------- Q > 1: MFMA tiles
// Workgroup (qt, split): queries [128 qt, +128) against candidate tiles [n_begin, n_end) of its split.  Wave w: candidates
// 64 (w & 1) .. +64, queries 64 (w >> 1) .. +64 of the tile, as 2 x 2 tiles of 32 x 32.  Lane l of a 32x32x2 MFMA holds A[i = l & 31][slot
// l >> 5] (candidate rows) and B[slot][j = l & 31] (queries): each lane loads float4s at k0 + 8t + 4h (h = l >> 5) of its candidate row and
// of its query, and feeds component s of the t-th float4 to MFMA step (t, s), so both operands of a slot always carry the same k.
// Every accumulator is one f32 fma chain over a fixed permutation of 128 consecutive k (exact products, one rounding each); the
// 128-k blocks are then added in k order (blocked summation: a C = 1024 score is 8 chains of 128 plus 8 adds, not one chain of 1024,
// which keeps the error of random unit vectors well inside 1.5e-7 sum|a b|).
struct MMFrag {
  float4 a[2][4];   // [candidate tile][t]
  float4 b[2][4];   // [query tile][t]
};

__device__ __forceinline__ void mm_load(MMFrag& f, const float* __restrict__ index, int64_t ld, const float* __restrict__ Qm, int C,
                                        int64_t n0, int64_t n_end, int q0, int Q, int k0, int lane, int w) {
  const int i = lane & 31, h = lane >> 5;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int64_t n = n0 + 64 * (w & 1) + 32 * m + i;
    const bool ok = n < n_end;
    const float* p = index + (ok ? n : 0) * ld;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int kk = k0 + 8 * t + 4 * h;
      f.a[m][t] = (ok && kk < C) ? *reinterpret_cast<const float4*>(p + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int qq = q0 + 64 * (w >> 1) + 32 * m + i;
    const bool ok = qq < Q;
    const float* p = Qm + (int64_t)(ok ? qq : 0) * C;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int kk = k0 + 8 * t + 4 * h;
      f.b[m][t] = (ok && kk < C) ? *reinterpret_cast<const float4*>(p + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
}

__device__ __forceinline__ float f4c(const float4& v, int s) { return s == 0 ? v.x : s == 1 ? v.y : s == 2 ? v.z : v.w; }

__global__ __launch_bounds__(256) void dot_topk_mfma_kernel(const float* __restrict__ index, int64_t ld, const float* __restrict__ Qm,
                                                            int N, int Q, int C, int k, int tiles_per_split, int nsplit,
                                                            uint64_t* __restrict__ parts) {
  extern __shared__ __attribute__((aligned(16))) uint64_t smem[];
  uint64_t* lists = smem;                                        // [k][128]: entry p of query j at p * 128 + j
  float* sc = reinterpret_cast<float*>(smem + (int64_t)k * MM_TILE);   // [128 candidates][128 queries]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int q0 = blockIdx.x * MM_TILE, split = blockIdx.y;
  const int64_t n_begin = (int64_t)split * tiles_per_split * MM_TILE;
  const int64_t n_end = min((int64_t)N, n_begin + (int64_t)tiles_per_split * MM_TILE);
  for (int e = threadIdx.x; e < k * MM_TILE; e += 256) lists[e] = 0;
  uint64_t thr = 0;                                              // the scanning thread's k-th entry
  const int n_tiles = n_begin < n_end ? (int)((n_end - n_begin + MM_TILE - 1) / MM_TILE) : 0;
  const int n_chunks = (C + 31) / 32;
  const int64_t iters = (int64_t)n_tiles * n_chunks;
  f32x16 acc[2][2], tot[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) acc[m][n] = tot[m][n] = f32x16{};
  MMFrag cur, nxt;
  if (iters > 0) mm_load(nxt, index, ld, Qm, C, n_begin, n_end, q0, Q, 0, lane, w);
  __syncthreads();
  for (int64_t it = 0; it < iters; ++it) {
    const int tile = (int)(it / n_chunks), chunk = (int)(it - (int64_t)tile * n_chunks);
    const int64_t n0 = n_begin + (int64_t)tile * MM_TILE;
    cur = nxt;
    if (it + 1 < iters) {
      const int t2 = (int)((it + 1) / n_chunks), c2 = (int)(it + 1 - (int64_t)t2 * n_chunks);
      mm_load(nxt, index, ld, Qm, C, n_begin + (int64_t)t2 * MM_TILE, n_end, q0, Q, 32 * c2, lane, w);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int n = 0; n < 2; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(f4c(cur.a[m][t], s), f4c(cur.b[n][t], s), acc[m][n], 0, 0, 0);
    if ((chunk & (MM_BLOCK_CHUNKS - 1)) == MM_BLOCK_CHUNKS - 1 || chunk == n_chunks - 1) {   // blocked summation: chains of 128 k
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          tot[m][n] += acc[m][n];
          acc[m][n] = f32x16{};
        }
    }
    if (chunk == n_chunks - 1) {
      // D[row = candidate][col = query]: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int cand = 64 * (w & 1) + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const int qq = 64 * (w >> 1) + 32 * n + (lane & 31);
            sc[cand * MM_TILE + qq] = tot[m][n][r];
            tot[m][n][r] = 0.f;
          }
      __syncthreads();
      if (threadIdx.x < MM_TILE && q0 + (int)threadIdx.x < Q) {
        const int j = threadIdx.x;
        const int valid = (int)min((int64_t)MM_TILE, n_end - n0);
        for (int c = 0; c < valid; ++c) {
          const uint64_t key = topk_key(sc[c * MM_TILE + j], (int)(n0 + c));
          if (key > thr) {
            int p = k - 1;
            while (p > 0 && lists[(p - 1) * MM_TILE + j] < key) {
              lists[p * MM_TILE + j] = lists[(p - 1) * MM_TILE + j];
              --p;
            }
            lists[p * MM_TILE + j] = key;
            thr = lists[(k - 1) * MM_TILE + j];
          }
        }
      }
      __syncthreads();
    }
  }
  if (threadIdx.x < MM_TILE && q0 + (int)threadIdx.x < Q) {
    const int j = threadIdx.x;
    uint64_t* dst = parts + ((int64_t)(q0 + j) * nsplit + split) * k;
    for (int p = 0; p < k; ++p) dst[p] = lists[p * MM_TILE + j];
  }
}

// ---------------------------------------------------------------------------------------------------------------- merge
// One workgroup per query: n_parts sorted lists of k keys -> the top k.  Each round every thread offers the best head of the lists it
// owns (list i belongs to thread i % 256), the workgroup takes the maximum key and its list advances.
__global__ __launch_bounds__(MERGE_THREADS) void dot_topk_merge_kernel(const uint64_t* __restrict__ parts, int n_parts, int k,
                                                                      float* __restrict__ scores, int* __restrict__ idx) {
  __shared__ int head[1024];
  __shared__ uint64_t red_key[MERGE_THREADS / 64];
  __shared__ int red_list[MERGE_THREADS / 64];
  const int q = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t* P = parts + (int64_t)q * n_parts * k;
  for (int i = threadIdx.x; i < n_parts; i += MERGE_THREADS) head[i] = 0;
  __syncthreads();
  for (int r = 0; r < k; ++r) {
    uint64_t best = 0;
    int bl = -1;
    for (int i = threadIdx.x; i < n_parts; i += MERGE_THREADS) {
      const int h = head[i];
      const uint64_t key = h < k ? P[(int64_t)i * k + h] : 0;
      if (key > best) best = key, bl = i;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint64_t ok = shfl_u64(best, lane ^ o);
      const int ol = __shfl_xor(bl, o, 64);
      if (ok > best) best = ok, bl = ol;
    }
    if (lane == 0) red_key[w] = best, red_list[w] = bl;
    __syncthreads();
    best = red_key[0], bl = red_list[0];
    for (int v = 1; v < MERGE_THREADS / 64; ++v)
      if (red_key[v] > best) best = red_key[v], bl = red_list[v];
    if (threadIdx.x == 0) {
      float s;
      int id;
      topk_unkey(best, &s, &id);
      scores[(int64_t)q * k + r] = s;
      idx[(int64_t)q * k + r] = id;
      if (bl >= 0) head[bl] += 1;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------- pool / normalise
// One workgroup per image: column sums of rows 1..S-1 in fp32, in row order; the mean rounded to bf16 (torch's bf16 mean), then
// divided by its fp32 L2 norm + 1e-12.
__global__ __launch_bounds__(256) void clip_pool_normalize_kernel(const bf16_t* __restrict__ x, int S, int C, float* __restrict__ out) {
  __shared__ float red[16];
  const bf16_t* p = x + (int64_t)blockIdx.x * S * C;
  float* o = out + (int64_t)blockIdx.x * C;
  float ss = 0.f;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float s = 0.f;
    for (int r = 1; r < S; ++r) s += bf2f(p[(int64_t)r * C + c]);
    const float m = bf2f(f2bf(s / (float)(S - 1)));
    o[c] = m;
    ss = fmaf(m, m, ss);
  }
  const float nrm = sqrtf(block_sum(ss, red)) + 1e-12f;
  for (int c = threadIdx.x; c < C; c += blockDim.x) o[c] = o[c] / nrm;
}

__global__ __launch_bounds__(256) void l2_normalize_rows_kernel(const float* __restrict__ x, float* __restrict__ out, int C) {
  __shared__ float red[16];
  const float* p = x + (int64_t)blockIdx.x * C;
  float* o = out + (int64_t)blockIdx.x * C;
  float ss = 0.f;
  for (int c = threadIdx.x; c < C; c += blockDim.x) ss = fmaf(p[c], p[c], ss);
  const float nrm = sqrtf(block_sum(ss, red)) + 1e-12f;
  for (int c = threadIdx.x; c < C; c += blockDim.x) o[c] = p[c] / nrm;
}

// ---------------------------------------------------------------------------------------------------------------- host
struct TopkPlan {
  int parts;             // partial lists per query
  int gemv_rows;         // Q == 1: rows per workgroup
  int tiles_per_split;   // Q > 1
};

TopkPlan topk_plan(int Q, int N) {
  TopkPlan pl{};
  if (Q == 1) {
    const int blocks = (int)std::min<int64_t>(GEMV_MAX_BLOCKS, std::max<int64_t>(1, mp_cdiv(N, 1024)));
    pl.gemv_rows = (int)mp_cdiv(mp_cdiv(N, blocks), 4 * GEMV_ROWS) * 4 * GEMV_ROWS;
    pl.parts = (int)mp_cdiv(N, pl.gemv_rows);
  } else {
    const int qtiles = (int)mp_cdiv(Q, MM_TILE);
    const int ntiles = (int)mp_cdiv(N, MM_TILE);
    const int want = (int)std::max<int64_t>(1, std::min<int64_t>(ntiles, mp_cdiv(MM_TARGET_BLOCKS, qtiles)));
    pl.tiles_per_split = (int)mp_cdiv(ntiles, want);
    pl.parts = (int)mp_cdiv(ntiles, pl.tiles_per_split);
  }
  return pl;
}

const char* topk_bad_shape(int64_t N, int64_t Q, int C, int k) {
  if (k < 1 || k > TK_MAX) return "k must be in [1, 64]";
  if (C <= 0 || C % 4) return "C must be a positive multiple of 4";
  if (N < 1 || N >= ((int64_t)1 << 31)) return "N must be in [1, 2^31)";
  if (Q < 1 || Q >= ((int64_t)1 << 31)) return "Q must be in [1, 2^31)";
  return nullptr;
}

}  // namespace

extern "C" int64_t mp_dot_topk_workspace_bytes(int64_t N, int64_t Q, int C, int k) {
  if (topk_bad_shape(N, Q, C, k)) return -1;
  return (int64_t)topk_plan((int)Q, (int)N).parts * Q * k * (int64_t)sizeof(uint64_t);
}

extern "C" int mp_dot_topk_f32(const float* index, int64_t ld_index, const float* queries, int64_t N, int64_t Q, int C, int k,
                               float* scores, int* idx, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  const char* bad = topk_bad_shape(N, Q, C, k);
  MP_REQUIRE(!bad, MP_ERR_SHAPE, "mp_dot_topk_f32: %s (N = %lld, Q = %lld, C = %d, k = %d)", bad, (long long)N, (long long)Q, C, k);
  MP_REQUIRE(ld_index >= C && ld_index % 4 == 0, MP_ERR_SHAPE, "mp_dot_topk_f32: ld_index %lld must be >= C and a multiple of 4",
             (long long)ld_index);
  MP_REQUIRE(index && queries && scores && idx && workspace, MP_ERR_ARG, "mp_dot_topk_f32: null operand");
  MP_REQUIRE(((uintptr_t)index & 15) == 0 && ((uintptr_t)queries & 15) == 0 && ((uintptr_t)workspace & 7) == 0, MP_ERR_ARG,
             "mp_dot_topk_f32: index and queries must be 16-byte aligned");
  const int64_t need = mp_dot_topk_workspace_bytes(N, Q, C, k);
  MP_REQUIRE(workspace_bytes >= need, MP_ERR_WORKSPACE, "mp_dot_topk_f32: workspace %lld < %lld bytes", (long long)workspace_bytes,
             (long long)need);
  const TopkPlan pl = topk_plan((int)Q, (int)N);
  uint64_t* parts = (uint64_t*)workspace;
  if (Q == 1) {
    hipLaunchKernelGGL(dot_topk_gemv_kernel, dim3((unsigned)pl.parts), dim3(256), 0, stream, index, ld_index, queries, (int)N, C, k,
                       pl.gemv_rows, parts);
    int rc = mp_check_launch("mp_dot_topk_f32(gemv)");
    if (rc) return rc;
  } else {
    const size_t lds = (size_t)k * MM_TILE * sizeof(uint64_t) + (size_t)MM_TILE * MM_TILE * sizeof(float);
    static bool attr = false;
    if (!attr) {
      (void)hipFuncSetAttribute((const void*)dot_topk_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(TK_MAX * MM_TILE * sizeof(uint64_t) + MM_TILE * MM_TILE * sizeof(float)));
      attr = true;
    }
    hipLaunchKernelGGL(dot_topk_mfma_kernel, dim3((unsigned)mp_cdiv(Q, MM_TILE), (unsigned)pl.parts), dim3(256), lds, stream, index,
                       ld_index, queries, (int)N, (int)Q, C, k, pl.tiles_per_split, pl.parts, parts);
    int rc = mp_check_launch("mp_dot_topk_f32(mfma)");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(dot_topk_merge_kernel, dim3((unsigned)Q), dim3(MERGE_THREADS), 0, stream, (const uint64_t*)parts, pl.parts, k,
                     scores, idx);
  return mp_check_launch("mp_dot_topk_f32(merge)");
}

extern "C" int mp_clip_pool_normalize_bf16(const void* hidden, int n, int S, int C, float* out, hipStream_t stream) {
  MP_REQUIRE(n > 0 && S > 1 && C > 0, MP_ERR_SHAPE, "mp_clip_pool_normalize_bf16: bad shape (n = %d, S = %d, C = %d; S >= 2)", n, S, C);
  MP_REQUIRE(hidden && out, MP_ERR_ARG, "mp_clip_pool_normalize_bf16: null operand");
  hipLaunchKernelGGL(clip_pool_normalize_kernel, dim3((unsigned)n), dim3(256), 0, stream, (const bf16_t*)hidden, S, C, out);
  return mp_check_launch("mp_clip_pool_normalize_bf16");
}

extern "C" int mp_l2_normalize_rows_f32(const float* x, float* out, int64_t rows, int C, hipStream_t stream) {
  MP_REQUIRE(rows > 0 && rows < ((int64_t)1 << 31) && C > 0, MP_ERR_SHAPE, "mp_l2_normalize_rows_f32: bad shape (rows = %lld, C = %d)",
             (long long)rows, C);
  MP_REQUIRE(x && out, MP_ERR_ARG, "mp_l2_normalize_rows_f32: null operand");
  hipLaunchKernelGGL(l2_normalize_rows_kernel, dim3((unsigned)rows), dim3(256), 0, stream, x, out, C);
  return mp_check_launch("mp_l2_normalize_rows_f32");
}
