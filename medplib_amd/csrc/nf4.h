// The NF4 weight format (QLoRA's 4-bit NormalFloat, bitsandbytes' load_in_4bit / bnb_4bit_quant_type="nf4") as this library stores it: the
// sixteen-entry table, the fifteen decision thresholds of the quantiser, and the table rounded to bf16 as the GEMV multiplies with it.
// A weight is a 4-bit code; 64 consecutive k of a row share one fp32 absmax; byte j of a row holds code[2j] << 4 | code[2j + 1].
// Everything here is constexpr, for host and device code alike; the tests restate the numbers by hand (tests/nf4_ref.py), on purpose.
// The GEMV's table entry of one BYTE of codes is the bf16 pair {hi nibble, lo nibble} as it lies against the x pair {x[2j], x[2j + 1]} in
// memory: the even k, which is the high nibble, in the low half of the dword (gemv_w4.hip, nq_fill).
#pragma once
#include <stdint.h>

constexpr int NF4_BLOCK = 64;                  // weights per absmax

constexpr float NF4[16] = {-1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f, -0.28444138169288635f,
                           -0.18477343022823334f, -0.09105003625154495f, 0.0f, 0.07958029955625534f, 0.16093020141124725f,
                           0.24611230194568634f, 0.33791524171829224f, 0.44070982933044434f, 0.5626170039176941f, 0.7229568362236023f, 1.0f};

// T[i]: a value above it (strictly) has a code above i.  The midpoint of two neighbours, taken in double and rounded once to fp32.
constexpr float nf4_threshold(int i) { return (float)(((double)NF4[i] + (double)NF4[i + 1]) / 2); }

// bf16(NF4[c]), round to nearest even, as its 16 bits.  The sixteen roundings stay distinct.
constexpr uint32_t nf4_bf16_bits(int c) {
  const uint32_t u = __builtin_bit_cast(uint32_t, NF4[c]);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// the four table entries 4q .. 4q + 3 as one 64-bit constant (entry c at bits 16 * (c & 3))
constexpr uint64_t nf4_quad_bits(int q) {
  return (uint64_t)nf4_bf16_bits(4 * q) | (uint64_t)nf4_bf16_bits(4 * q + 1) << 16 | (uint64_t)nf4_bf16_bits(4 * q + 2) << 32 |
         (uint64_t)nf4_bf16_bits(4 * q + 3) << 48;
}

#ifdef __HIPCC__
// bf16(NF4[c]) bits for a run-time code, from immediates (no table in memory: this fills the LDS table at the head of every GEMV launch,
// where a constant-memory load would be a round trip ahead of the weight stream)
__device__ __forceinline__ uint32_t nf4_bf16_bits_dev(uint32_t c) {
  const uint32_t q = c >> 2;
  const uint64_t lo = q & 1 ? nf4_quad_bits(1) : nf4_quad_bits(0), hi = q & 1 ? nf4_quad_bits(3) : nf4_quad_bits(2);
  return (uint32_t)((q & 2 ? hi : lo) >> (16 * (c & 3))) & 0xffffu;
}

// the quantiser's decision: the number of thresholds strictly below v (a tie goes to the lower code)
__device__ __forceinline__ uint32_t nf4_code(float v) {
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 15; ++i) c += v > nf4_threshold(i) ? 1u : 0u;
  return c;
}
#endif
