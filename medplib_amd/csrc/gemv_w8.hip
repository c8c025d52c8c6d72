// 8-bit-weight GEMV for the single-token decode steps (the reference worker's --load-8bit: model/serve/model_worker.py:72,100,642 ->
// builder.py:39, bitsandbytes Linear8bitLt): y[m, n] = epilogue(scale[n] * sum_k code[n, k] * x[m, k]) for M <= 8 rows of bf16 x against int8
// codes with one fp32 scale per output row (row-wise absmax, bitsandbytes' weight format; the activations stay bf16: W8A16).  A decode step
// is a weight stream, so halving the bytes of W is what this buys.  mp_gemv_w8_bf16 is the int8 policy of the three forms of gemv_forms.h
// (kernels, the code stream gq_stream and the host dispatch are there, shared with mp_gemv_bf16); this file holds the entry point and the
// quantiser.  Measured: profiles/w8_decode.md.
#include "gemv_forms.h"

namespace {

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
  MP_REQUIRE(M >= 1 && M <= GV_MAXM && N > 0 && K > 0 && K % 16 == 0 && ldx % 8 == 0 && ldw % 16 == 0 && strideW % 16 == 0, MP_ERR_SHAPE,
             "mp_gemv_w8_bf16: 1 <= M <= 8, K %% 16 == 0 (M=%d N=%d K=%d)", M, N, K);
  MP_REQUIRE(out_dtype == MP_BF16 || out_dtype == MP_F32, MP_ERR_DTYPE, "mp_gemv_w8_bf16: bad out dtype");
  MP_REQUIRE(!bias, MP_ERR_ARG, "mp_gemv_w8_bf16: no bias (no decode projection has one)");
  MP_REQUIRE(act == ACT_NONE || act == ACT_SWIGLU_PAIR, MP_ERR_ARG, "mp_gemv_w8_bf16: activation NONE or SWIGLU_PAIR only (%d)", act);
  MP_REQUIRE(act != ACT_SWIGLU_PAIR || (N % 64 == 0 && out_dtype == MP_BF16 && !residual), MP_ERR_ARG,
             "mp_gemv_w8_bf16: SWIGLU_PAIR needs N %% 64 == 0, bf16 output, no residual");
  MP_REQUIRE(!w_index || out_dtype == MP_BF16, MP_ERR_ARG, "mp_gemv_w8_bf16: the indexed (expert) form writes bf16");
  MP_REQUIRE(x && W && scale && y, MP_ERR_ARG, "mp_gemv_w8_bf16: null operand");
  GemvArgsT<int8_t> g{(const bf16_t*)x, ldx, (const int8_t*)W, ldw, strideW, y, ldy, nullptr, (const bf16_t*)residual, ldr, w_index, row_scale,
                      row_keep, M, N, K, act, out_dtype == MP_F32, alpha, scale, strideScale};
  static const char* const names[3] = {"mp_gemv_w8_bf16", "mp_gemv_w8_bf16(indexed)", "mp_gemv_w8_bf16(ksplit)"};
  return gemv_launch<WeightInt8>(g, stream, names);
}
