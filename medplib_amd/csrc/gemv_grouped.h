// What the grouped expert GEMVs of every weight type share (gemv_grouped.hip: bf16 and int8; gemv_w4.hip: NF4): the argument block's expert
// count, the sorting of a launch's rows into passes and the x rows of a pass.
#pragma once
#include "gemv_forms.h"

namespace {

template <class T>
struct GroupedArgsT {
  GemvArgsT<T> g;
  int E;
};
using GroupedArgs = GroupedArgsT<bf16_t>;

// The rows of a launch as a wave sees them: `todo` = the kept rows still to be computed, `dead` = the rows that stream nothing (row_keep < 0, or
// an expert index outside [0, E): such a row is stored as a dropped one instead of reading past the weight tensor).  Wave-uniform.
struct GroupedRows {
  int ev;                          // lane m < M: w_index[m]
  bool live;                       // lane m: row m is kept
  unsigned long long todo, dead;
  template <class A>
  __device__ __forceinline__ GroupedRows(const A& a, int lane) {
    const auto& g = a.g;
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

template <int NR, class Args>
__device__ __forceinline__ void gg_x_rows(const Args& g, unsigned sel, const bf16_t* (&xp)[NR]) {
#pragma unroll
  for (int j = 0; j < NR; ++j) xp[j] = g.x + (int64_t)((sel >> (4 * j)) & 15u) * g.ldx;
}

// The x rows of a pass over top-2 entries (mp_moe_route_top2's layout, entry e = c * T + t): entry e reads its token's row, e % T.
template <int NR, class Args>
__device__ __forceinline__ void gg_x_rows_top2(const Args& g, unsigned sel, int T, const bf16_t* (&xp)[NR]) {
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int m = (sel >> (4 * j)) & 15u;
    xp[j] = g.x + (int64_t)(m >= T ? m - T : m) * g.ldx;
  }
}

// The passes of next() as they come: up to four rows.
#define MP_GG_PASSES_OF_FOUR(cnt, sel, PASS)       \
  do {                                             \
    switch (cnt) {                                 \
      case 1: PASS(1, sel); break;                 \
      case 2: PASS(2, sel); break;                 \
      case 3: PASS(3, sel); break;                 \
      default: PASS(4, sel);                       \
    }                                              \
  } while (0)

// A kernel whose passes hold at most two rows takes next()'s pass of three or four as two passes, in the same ascending row order.
#define MP_GG_PASSES_OF_TWO(cnt, sel, PASS)        \
  do {                                             \
    switch (cnt) {                                 \
      case 1: PASS(1, sel); break;                 \
      case 2: PASS(2, sel); break;                 \
      case 3: PASS(2, sel); PASS(1, (sel) >> 8); break; \
      default: PASS(2, sel); PASS(2, (sel) >> 8);  \
    }                                              \
  } while (0)

}  // namespace
