// Temperature sampling of the next token on the device (the serving worker's softmax(logits / T) + multinomial pick; greedy decoding keeps
// mp_argmax_rows_f32 in norm_elementwise.hip).  gfx950, wave64.
#include "common.h"

namespace {

// Inverse-CDF pick of one column per row: w_j = exp((l_j - max l) / T), out = the smallest i with w_i > 0 whose cumulative weight C(i)
// exceeds u * C(cols - 1).  One block of 1024 threads per row, K float4 pieces per thread (piece p = tid + k * 1024 covers columns
// 4p .. 4p + 3, so a wave's 64 pieces are 1 KB of consecutive columns: one 16-byte load per piece when the row starts on 16 bytes — the decode row
// does — and four 4-byte loads at a 16-byte lane stride otherwise, over the same 1 KB); up to 32768 columns the row
// stays in registers after the one read, wider rows (K = 16) are read again from L2 in steps 2 and 3:
//   1. row maximum (block reduction), weights in place of the logits;
//   2. the sum of every piece in a fixed order ((w0 + w1) + w2) + w3, an inclusive scan of the 64 piece sums of every (k, wave) chunk
//      (Hillis-Steele over the lanes), the 16 K chunk totals scanned by wave 0 — the cumulative weight in front of every piece;
//   3. C(i) = chunk base + lane base + the piece's running sum.  Every thread compares the C of its own columns with the target, which is
//      the scan inside the chunk that holds the target without reading the row again: the pieces of every other chunk lie wholly on one side
//      of the target and yield no candidate (up to the rounding of C, below).  The block takes the smallest candidate.
// No atomics and no order that depends on timing: the same row, u and T give the same column on every launch, for every alignment of the row
// (a row that does not start on 16 bytes — rows of a batch with an odd ld — is read column by column into the SAME registers: a unit-stride
// read over the lanes would change which thread sums which columns, and with it the last bits of C) and whatever rows share the launch.
// C is an fp32 sum whose grouping changes at piece, lane and chunk borders, so it may dip by an ulp of the total at such a border; "smallest i
// with C(i) > target and w_i > 0" is well defined all the same, and every i in front of the pick has C(i) <= target.  If no column qualifies
// (u >= 1 — the keyed generator does return exactly 1.0, see include/medplib_hip.h — or u so close to 1 that rounding leaves the last C at or
// below the target; also a NaN u) the pick is the LAST column with w > 0; u <= 0 gives the first.  A row without any w > 0 (all -inf, all
// NaN) gives 0; NaN columns beside finite ones weigh nothing and make C NaN, which ends at the last column with w > 0.  Columns at or past `cols` carry w = 0 and are never picked.
__device__ __forceinline__ float lane_scan_step(float v, int o, int lane) {
  const float t = __shfl_up(v, o, 64);
  return lane >= o ? v + t : v;
}

template <int K, bool KEEP>
__global__ __launch_bounds__(1024) void sample_rows_kernel(const float* __restrict__ x, int64_t ld, int cols, float inv_t,
                                                           const float* __restrict__ u, int64_t* __restrict__ out) {
  constexpr int NC = 16 * K;                 // chunks of 64 pieces (256 columns): chunk c = k * 16 + wave, in column order
  __shared__ float red[16];
  __shared__ float chunk_sum[NC];            // totals, then the cumulative weight in front of each chunk
  __shared__ float total_s;
  __shared__ int first_s[16], last_s[16];
  const float* r = x + (int64_t)blockIdx.x * ld;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool wide = (reinterpret_cast<uintptr_t>(r) & 15) == 0;       // (block-uniform)

  auto piece = [&](int k) {
    const int i = 4 * (tid + k * 1024);
    float4 p;
    if (wide && i + 3 < cols) {
      p = *reinterpret_cast<const float4*>(r + i);
    } else {                                 // the piece that straddles `cols`, pieces past it, and rows off 16 bytes
      p.x = i < cols ? r[i] : -INFINITY;
      p.y = i + 1 < cols ? r[i + 1] : -INFINITY;
      p.z = i + 2 < cols ? r[i + 2] : -INFINITY;
      p.w = i + 3 < cols ? r[i + 3] : -INFINITY;
    }
    return p;
  };
  float4 v[K];                               // KEEP: the row, then its weights, stay in registers
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float4 p = piece(k);
    if (KEEP) v[k] = p;
    m = fmaxf(m, fmaxf(fmaxf(p.x, p.y), fmaxf(p.z, p.w)));
  }
  m = block_max(m, red);

  // a column equal to the maximum has w = 1 exactly (also when the maximum is +inf, where l - max is not a number).  Columns at or past `cols`
  // (loaded as -inf) and every column of a row without a maximum above -inf (all -inf, all NaN) weigh 0, whatever they compare equal to.
  const bool has_max = m > -INFINITY;
  auto weight = [&](float l, int i) { return (has_max && i < cols) ? (l == m ? 1.f : __expf((l - m) * inv_t)) : 0.f; };
  auto weights = [&](float4 p, int k) {
    const int i = 4 * (tid + k * 1024);
    p.x = weight(p.x, i); p.y = weight(p.y, i + 1); p.z = weight(p.z, i + 2); p.w = weight(p.w, i + 3);
    return p;
  };
  float incl[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float4 w = weights(KEEP ? v[k] : piece(k), k);
    if (KEEP) v[k] = w;
    incl[k] = ((w.x + w.y) + w.z) + w.w;
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) incl[k] = lane_scan_step(incl[k], o, lane);
  }
  if (lane == 63) {
#pragma unroll
    for (int k = 0; k < K; ++k) chunk_sum[k * 16 + wave] = incl[k];
  }
  __syncthreads();
  if (wave == 0) {                           // NC / 64 consecutive chunks per lane, then a scan over the lanes
    constexpr int PER = NC / 64;
    float s[PER], run = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) { s[j] = chunk_sum[lane * PER + j]; run += s[j]; }
    float inc = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) inc = lane_scan_step(inc, o, lane);
    float base = __shfl_up(inc, 1, 64);      // the cumulative weight in front of this lane's chunks
    if (lane == 0) base = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) { chunk_sum[lane * PER + j] = base; base += s[j]; }
    if (lane == 63) total_s = inc;
  }
  __syncthreads();
  const float target = u[blockIdx.x] * total_s;

  int first = 0x7fffffff, last = -1;         // smallest qualifying column of this thread; its last column with w > 0
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float prev = __shfl_up(incl[k], 1, 64);
    if (lane == 0) prev = 0.f;
    const float base = chunk_sum[k * 16 + wave] + prev;
    const int i = 4 * (tid + k * 1024);
    const float4 w = KEEP ? v[k] : weights(piece(k), k);      // (the same expression on the same logits: the same bits as in step 2)
    const float c0 = base + w.x, c1 = base + (w.x + w.y), c2 = base + ((w.x + w.y) + w.z), c3 = base + (((w.x + w.y) + w.z) + w.w);
    if (w.w > 0.f) { last = max(last, i + 3); if (c3 > target) first = min(first, i + 3); }
    if (w.z > 0.f) { last = max(last, i + 2); if (c2 > target) first = min(first, i + 2); }
    if (w.y > 0.f) { last = max(last, i + 1); if (c1 > target) first = min(first, i + 1); }
    if (w.x > 0.f) { last = max(last, i); if (c0 > target) first = min(first, i); }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    first = min(first, __shfl_xor(first, o, 64));
    last = max(last, __shfl_xor(last, o, 64));
  }
  if (lane == 0) { first_s[wave] = first; last_s[wave] = last; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 16; ++w) { first = min(first, first_s[w]); last = max(last, last_s[w]); }
    out[blockIdx.x] = min(first != 0x7fffffff ? first : (last >= 0 ? last : 0), cols - 1);      // (the clamp never binds: w = 0 past cols)
  }
}

}  // namespace

extern "C" int mp_sample_rows_f32(const float* logits, int64_t ld, int64_t rows, int cols, float inv_temperature, const float* u, int64_t* out,
                                  hipStream_t stream) {
  MP_REQUIRE(cols > 0 && cols <= 65536 && rows >= 0, MP_ERR_SHAPE, "mp_sample_rows_f32: bad shape (rows=%lld cols=%d; 0 < cols <= 65536)",
             (long long)rows, cols);
  MP_REQUIRE(inv_temperature > 0.f && inv_temperature <= 3.402823466e38f, MP_ERR_SHAPE, "mp_sample_rows_f32: inv_temperature=%g must be positive and finite",
             (double)inv_temperature);
  if (rows == 0) return MP_OK;
  MP_REQUIRE(logits != nullptr && u != nullptr && out != nullptr, MP_ERR_ARG, "mp_sample_rows_f32: null operand");
  MP_REQUIRE(rows == 1 || ld >= cols || ld == 0, MP_ERR_SHAPE, "mp_sample_rows_f32: ld=%lld < cols=%d (ld = 0: one row against every u)",
             (long long)ld, cols);
  if (cols <= 32768)                         // the decode row (32000 + added tokens): 8 float4 per thread, held in registers
    hipLaunchKernelGGL((sample_rows_kernel<8, true>), dim3((unsigned)rows), dim3(1024), 0, stream, logits, ld, cols, inv_temperature, u, out);
  else                                       // 16 pieces per thread do not fit the 128 registers of a 1024-thread block: the row is read three times (L2)
    hipLaunchKernelGGL((sample_rows_kernel<16, false>), dim3((unsigned)rows), dim3(1024), 0, stream, logits, ld, cols, inv_temperature, u, out);
  return mp_check_launch("mp_sample_rows_f32");
}
