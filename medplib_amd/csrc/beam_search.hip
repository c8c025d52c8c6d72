// Beam search between two decode steps, on the device (HF 4.31 GenerationMixin.beam_search; the reference's vqa_infer.py:430-442 passes
// --num_beams to generate()): the candidate selection over the nb beams' next-token logits, and the re-order of the KV cache by the chosen
// parents (HF's _reorder_cache).  gfx950, wave64.  Both launches are capturable: no host read, no allocation.
#include "row_pick.h"

#include <algorithm>

namespace {

constexpr int BEAM_MAX = 8;                  // beams per launch; 2 * BEAM_MAX candidates leave every row
constexpr int CAND_MAX = 2 * BEAM_MAX;

// The rows' candidates between the two launches of mp_beam_topk_f32: [beam][rank] keys (below), 0 = no candidate.  One copy per device (a
// module global), shared by every stream: calls on different streams of one device must not overlap.
__device__ unsigned long long g_row_cands[BEAM_MAX * CAND_MAX];

// A candidate as ONE unsigned 64-bit key whose order is the ranking: the order-preserving integer image of the value (row_pick::float_key) in
// the high word (larger value first), the complement of the flat index b * cols + c in the low word (lower index first among equal values).
// -0 is folded onto +0, so equal values have equal high words.  Valid keys are > 0 (the image of -inf is 0x007fffff); 0 stands for "none".
__device__ __forceinline__ unsigned long long cand_key(float v, unsigned flat) {
  if (__float_as_uint(v) == 0x80000000u) v = 0.f;
  return ((unsigned long long)row_pick::float_key(v) << 32) | (unsigned long long)(~flat);
}
__device__ __forceinline__ float key_value(unsigned long long key) { return row_pick::key_float((unsigned)(key >> 32)); }
__device__ __forceinline__ unsigned key_flat(unsigned long long key) { return ~(unsigned)key; }

// Launch 1: one block per beam in the geometry of row_pick.h (up to 32768 columns the row stays in registers, wider rows are read again from
// L2 in every round).
//   m = the row maximum, Z = sum exp(l - m): NaN columns are left out of both (and are never candidates).  A row whose maximum is not finite
//   (all -inf, all NaN, a +inf) has no candidates.
//   v(c) = ((l_c - m) - log Z) + score: fp32; Z is summed in ONE fixed order (a thread's columns in order, then row_pick::block_sum's), so v
//   has the same bits on every launch, for every alignment of the row.
//   2 * nb rounds of a block arg-max over the keys strictly below the previous pick: the row's 2 * nb best in rank order, ties by construction.
template <int K, bool KEEP>
__global__ __launch_bounds__(1024) void beam_row_topk_kernel(const float* __restrict__ x, int64_t ld, int nb, int cols,
                                                             const float* __restrict__ beam_scores) {
  using namespace row_pick;
  __shared__ unsigned redf[2][16];
  __shared__ unsigned long long redk[2][16];
  const int beam = blockIdx.x, tid = threadIdx.x;
  const float* r = x + (int64_t)beam * ld;
  const bool wide = starts_on_16_bytes(r);
  auto piece = [&](int k) { return load_piece(r, wide, cols, __uint_as_float(0x7fc00000u), k); };      // columns at or past `cols`: NaN
  const float score = beam_scores[beam];
  int phase = 0, kphase = 0;

  float4 v[KEEP ? K : 1];
  constexpr int UN = unroll_of(K, KEEP);
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float4 p = piece(k);
    if constexpr (KEEP) v[k] = p;
    m = fmaxf(m, piece_max(p));
  }
  m = block_fmax(m, redf, phase);
  unsigned long long* out = g_row_cands + beam * CAND_MAX;
  if (!(m > -INFINITY && m < INFINITY)) {                       // no candidates (block-uniform)
    if (tid < 2 * nb) out[tid] = 0ull;
    return;
  }
  auto w = [&](float l) { return l == l ? __expf(l - m) : 0.f; };
  float z = 0.f;
#pragma unroll UN
  for (int k = 0; k < K; ++k) {
    const float4 p = KEEP ? v[KEEP ? k : 0] : piece(k);
    z += ((w(p.x) + w(p.y)) + w(p.z)) + w(p.w);
  }
  const float logz = logf(block_sum(z, redf, phase));
  auto value = [&](float l) { return ((l - m) - logz) + score; };       // NaN for a NaN column (and the padding)
  if constexpr (KEEP) {
#pragma unroll
    for (int k = 0; k < K; ++k) { v[k].x = value(v[k].x); v[k].y = value(v[k].y); v[k].z = value(v[k].z); v[k].w = value(v[k].w); }
  }
  const unsigned flat0 = (unsigned)beam * (unsigned)cols;
  unsigned long long prev = ~0ull;            // above every key
  for (int round = 0; round < 2 * nb; ++round) {
    unsigned long long best = 0ull;
#pragma unroll UN
    for (int k = 0; k < K; ++k) {
      float4 p;
      if constexpr (KEEP) {
        p = v[k];
      } else {
        p = piece(k);
        p.x = value(p.x); p.y = value(p.y); p.z = value(p.z); p.w = value(p.w);
      }
      const unsigned i = flat0 + (unsigned)piece_column(k);
      const float e[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned long long key = e[j] == e[j] ? cand_key(e[j], i + j) : 0ull;
        if (key < prev && key > best) best = key;
      }
    }
    best = block_all_reduce(best, 0ull, [](unsigned long long a, unsigned long long b) { return b > a ? b : a; }, redk, kphase);
    if (tid == 0) out[round] = best;
    if (best == 0ull) {                       // the row ran out of candidates (block-uniform): the rest are none
      if (tid > round && tid < 2 * nb) out[tid] = 0ull;
      return;
    }
    prev = best;
  }
}

// Launch 2: one wave merges the nb x 2 nb row candidates by rank (a key's rank = the number of larger keys: the keys are distinct), then lane 0
// walks the 2 nb best in rank order as BeamSearchScorer.process does: candidates whose token is eos_id are skipped, the first nb of the rest
// continue.  Unfilled candidates: index -1, score -inf, MP_POS_ERR_BEAM; continuations that cannot be filled from them: token 0, parent 0, -inf.
__global__ __launch_bounds__(64) void beam_merge_kernel(int nb, int cols, int eos_id, float* __restrict__ cand_score, int* __restrict__ cand_index,
                                                        float* next_scores, int64_t* __restrict__ next_tokens, int* __restrict__ next_parent,
                                                        int* __restrict__ err) {
  __shared__ unsigned long long all[BEAM_MAX * CAND_MAX], top[CAND_MAX];
  const int lane = threadIdx.x, n = nb * 2 * nb;
  for (int j = lane; j < n; j += 64) all[j] = g_row_cands[(j / (2 * nb)) * CAND_MAX + j % (2 * nb)];
  if (lane < CAND_MAX) top[lane] = 0ull;
  __syncthreads();
  for (int j = lane; j < n; j += 64) {
    const unsigned long long mine = all[j];
    if (mine == 0ull) continue;
    int rank = 0;
    for (int i = 0; i < n; ++i) rank += all[i] > mine;
    if (rank < 2 * nb) top[rank] = mine;
  }
  __syncthreads();
  if (lane != 0) return;
  int taken = 0;
  bool unfilled = false;
  for (int rk = 0; rk < 2 * nb; ++rk) {
    const unsigned long long key = top[rk];
    if (key == 0ull) {
      cand_score[rk] = -INFINITY;
      cand_index[rk] = -1;
      unfilled = true;
      continue;
    }
    const float s = key_value(key);
    const int flat = (int)key_flat(key), tok = flat % cols;
    cand_score[rk] = s;
    cand_index[rk] = flat;
    if (tok != eos_id && taken < nb) {
      next_scores[taken] = s;
      next_tokens[taken] = tok;
      next_parent[taken] = flat / cols;
      ++taken;
    }
  }
  for (; taken < nb; ++taken) {
    next_scores[taken] = -INFINITY;
    next_tokens[taken] = 0;
    next_parent[taken] = 0;
  }
  if (unfilled) atomicOr(err, MP_POS_ERR_BEAM);
}

// One thread owns one 16-byte column slice of one (tensor, position) across all nb beams: it loads the nb slices it is going to store (row
// parent[b] for row b), then stores those that move.  Nobody else touches these bytes: no hazard, no barrier.  The positions are
// lo <= p < min(*hi_dev, cache_rows), read on the device; the grid is sized for the whole tail and walks (tensor, position, slice) with the
// slice fastest.  An entry of `parent` outside [0, nb): nothing is written anywhere, MP_POS_ERR_BEAM; a null or misaligned table entry: that
// tensor is left alone, MP_POS_ERR_BEAM.
__global__ __launch_bounds__(256) void kv_permute_rows_kernel(bf16_t* const* __restrict__ tensors, int n, const int* __restrict__ parent, int nb,
                                                              int64_t batch_stride, int row_elems, int lo, const int* __restrict__ hi_dev,
                                                              int cache_rows, int* __restrict__ err) {
  int par[BEAM_MAX];
  bool bad = false, identity = true;
#pragma unroll
  for (int b = 0; b < BEAM_MAX; ++b) {
    par[b] = b < nb ? parent[b] : b;
    bad |= b < nb && (par[b] < 0 || par[b] >= nb);
    identity &= par[b] == b;
  }
  if (bad) {                                 // (grid-uniform)
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(err, MP_POS_ERR_BEAM);
    return;
  }
  const int hi = min(*hi_dev, cache_rows);
  if (identity || hi <= lo) return;
  const int64_t slices = row_elems / 8, span = hi - lo, total = (int64_t)n * span * slices;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t s = idx % slices, rest = idx / slices, p = lo + rest % span;
    bf16_t* base = tensors[rest / span];
    if (base == nullptr || (reinterpret_cast<uintptr_t>(base) & 15) != 0) {
      if (s == 0 && p == lo) atomicOr(err, MP_POS_ERR_BEAM);
      continue;
    }
    bf16_t* at = base + p * row_elems + s * 8;
    bf16x8 v[BEAM_MAX];
#pragma unroll
    for (int b = 0; b < BEAM_MAX; ++b)
      if (b < nb) v[b] = *reinterpret_cast<const bf16x8*>(at + par[b] * batch_stride);
#pragma unroll
    for (int b = 0; b < BEAM_MAX; ++b)
      if (b < nb && par[b] != b) *reinterpret_cast<bf16x8*>(at + b * batch_stride) = v[b];
  }
}

}  // namespace

extern "C" int mp_beam_topk_f32(const float* logits, int64_t ld, int nb, int cols, const float* beam_scores, int eos_id, float* cand_score,
                                int* cand_index, float* next_scores, int64_t* next_tokens, int* next_parent, int* err, hipStream_t stream) {
  MP_REQUIRE(nb >= 1 && nb <= BEAM_MAX && cols >= 2 && cols <= 65536, MP_ERR_SHAPE,
             "mp_beam_topk_f32: bad shape (nb=%d cols=%d; 1 <= nb <= 8, 2 <= cols <= 65536)", nb, cols);
  MP_REQUIRE(ld >= cols || ld == 0, MP_ERR_SHAPE, "mp_beam_topk_f32: ld=%lld < cols=%d (ld = 0: every beam reads the same row)", (long long)ld, cols);
  MP_REQUIRE(logits && beam_scores && cand_score && cand_index && next_scores && next_tokens && next_parent && err, MP_ERR_ARG,
             "mp_beam_topk_f32: null operand");
  row_pick::for_width(cols, [&](auto shape) {
    using S = decltype(shape);
    hipLaunchKernelGGL((beam_row_topk_kernel<S::K, S::KEEP>), dim3((unsigned)nb), dim3(1024), 0, stream, logits, ld, nb, cols, beam_scores);
  });
  hipLaunchKernelGGL(beam_merge_kernel, dim3(1), dim3(64), 0, stream, nb, cols, eos_id, cand_score, cand_index, next_scores, next_tokens, next_parent,
                     err);
  return mp_check_launch("mp_beam_topk_f32");
}

extern "C" int mp_kv_permute_rows_bf16(const void* tensors, int n, const int* parent, int nb, int64_t batch_stride, int64_t row_elems, int lo,
                                       const int* hi_dev, int cache_rows, int* err, hipStream_t stream) {
  MP_REQUIRE(n >= 0 && n <= 65535 && nb >= 1 && nb <= BEAM_MAX, MP_ERR_SHAPE, "mp_kv_permute_rows_bf16: bad shape (n=%d nb=%d; 0 <= n <= 65535, 1 <= nb <= 8)",
             n, nb);
  MP_REQUIRE(row_elems > 0 && row_elems % 8 == 0 && row_elems <= (1 << 24), MP_ERR_SHAPE,
             "mp_kv_permute_rows_bf16: row_elems=%lld must be a positive multiple of 8 (at most 2^24)", (long long)row_elems);
  MP_REQUIRE(cache_rows > 0 && lo >= 0 && batch_stride % 8 == 0 && batch_stride >= (int64_t)cache_rows * row_elems, MP_ERR_SHAPE,
             "mp_kv_permute_rows_bf16: cache_rows=%d > 0, lo=%d >= 0, batch_stride=%lld a multiple of 8 and >= cache_rows * row_elems", cache_rows, lo,
             (long long)batch_stride);
  if (n == 0) return MP_OK;
  MP_REQUIRE(tensors && parent && hi_dev && err, MP_ERR_ARG, "mp_kv_permute_rows_bf16: null operand");
  if (lo >= cache_rows) return MP_OK;         // no position can qualify
  // memory-bound: at most 4096 workgroups, the rest by the walk; *hi_dev is not known here, so the grid is sized for the whole tail
  const int64_t threads = (int64_t)n * (cache_rows - lo) * (row_elems / 8);
  const int64_t blocks = std::min<int64_t>(4096, mp_cdiv(threads, 256));
  hipLaunchKernelGGL(kv_permute_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (bf16_t* const*)tensors, n, parent, nb, batch_stride,
                     (int)row_elems, lo, hi_dev, cache_rows, err);
  return mp_check_launch("mp_kv_permute_rows_bf16");
}
