// Host side of the bf16 MFMA GEMM: everything that decides WHICH tile kernel a call gets (128x128, 256x256 or 320x256) and all C-ABI entry
// points.  The kernels and their launchers are gemm_bf16.hip (mp_launch_gemm128), gemm256_bf16.hip (mp_launch_gemm256) and gemm320_bf16.hip
// (mp_launch_gemm320, plus mp_gemm320_eligible / mp_gemm320_subwave_split, which know that kernel's tile constants and epilogue families).
// In order: the split-K workspace registry, the environment switches, the selection rules, dispatch_gemm() and the entry points.
#include "gemm_common.h"
#include <stdlib.h>
#include <algorithm>
#include <map>
#include <mutex>
#include <utility>

constexpr int BK = 64;          // the K step of all three kernels

// split-K workspaces, registered by the host: >= n_cu * 256 KiB of fp32 partials + >= 384 tickets each (the 320-row kernel keeps three words per tail tile).  One workspace serves
// one stream at a time, so a stream that runs GEMMs concurrently with others registers its own (mp_gemm_set_stream_workspace);
// launches on any other stream of that device use the device's default entry (mp_gemm_set_workspace).  The table is keyed by
// (device, stream) with no cap on either; it is only a directory of caller-owned buffers (the library never allocates).
struct SplitWs { float* ws; int* tickets; int64_t bytes; };
static std::mutex g_split_mu;
static std::map<std::pair<int, hipStream_t>, SplitWs> g_split;          // stream == nullptr: the device's default entry

static int current_device() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  return dev;
}

static int register_split_ws(hipStream_t stream, void* ws, int64_t ws_bytes, int* tickets) {
  std::lock_guard<std::mutex> lk(g_split_mu);
  const auto key = std::make_pair(current_device(), stream);
  if (ws) g_split[key] = SplitWs{(float*)ws, tickets, ws_bytes};
  else g_split.erase(key);
  return MP_OK;
}

extern "C" int mp_gemm_set_workspace(void* ws, int64_t ws_bytes, int* tickets, int n_tickets) {
  MP_REQUIRE(ws == nullptr || (tickets != nullptr && n_tickets >= 384), MP_ERR_ARG, "mp_gemm_set_workspace: need >= 384 zeroed int tickets");
  return register_split_ws(nullptr, ws, ws_bytes, tickets);
}

extern "C" int mp_gemm_set_stream_workspace(hipStream_t stream, void* ws, int64_t ws_bytes, int* tickets, int n_tickets) {
  MP_REQUIRE(ws == nullptr || (tickets != nullptr && n_tickets >= 384), MP_ERR_ARG, "mp_gemm_set_stream_workspace: need >= 384 zeroed int tickets");
  MP_REQUIRE(stream != nullptr, MP_ERR_ARG, "mp_gemm_set_stream_workspace: the default entry is mp_gemm_set_workspace");
  return register_split_ws(stream, ws, ws_bytes, tickets);
}

void mp_gemm_split_workspace(hipStream_t stream, float** ws, int** tickets, int64_t* bytes) {
  std::lock_guard<std::mutex> lk(g_split_mu);
  const int dev = current_device();
  auto it = g_split.find(std::make_pair(dev, stream));
  if (it == g_split.end()) it = g_split.find(std::make_pair(dev, (hipStream_t) nullptr));
  if (it == g_split.end()) { *ws = nullptr; *tickets = nullptr; *bytes = 0; return; }
  *ws = it->second.ws; *tickets = it->second.tickets; *bytes = it->second.bytes;
}

// Whether `stream` has its own registered workspace, i.e. the host declared that it runs GEMMs CONCURRENTLY with the device's primary
// stream.  The 320-row kernel's cooperative tail (units that WAIT for their siblings) is only deadlock-free while a single kernel on
// the device waits at a time: two such kernels on two streams can each hold CUs the other's missing units need.
bool mp_gemm_stream_registered(hipStream_t stream) {
  if (!stream) return false;
  std::lock_guard<std::mutex> lk(g_split_mu);
  return g_split.find(std::make_pair(current_device(), stream)) != g_split.end();
}

// CU count of the CURRENT device (immutable per device; cached per device id, not in a process-wide static)
int mp_device_cus() {
  static std::mutex mu;
  static std::map<int, int> cus;
  const int dev = current_device();
  std::lock_guard<std::mutex> lk(mu);
  auto it = cus.find(dev);
  if (it != cus.end()) return it->second;
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  cus[dev] = n;
  return n;
}

int mp_gemm_variant() {
  static int v = -1;
  if (v < 0) {
    // 2 (default) = auto: 256x256 ping-pong kernel for large problems, 128x128 LDS-DMA kernel otherwise;
    // 1 = always 128x128 LDS-DMA staging; 0 = 128x128 register staging (A/B reference)
    const char* e = getenv("MP_GEMM_VARIANT");
    v = (e && e[0] >= '0' && e[0] <= '2') ? (e[0] - '0') : 2;
  }
  return v;
}

static int gemm_group_m() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("MP_GEMM_GROUP_M");
    v = (e && atoi(e) >= 1) ? atoi(e) : 4;
  }
  return v;
}

static bool use_256_rule(const GemmArgs& g, int batch) {
  if (g.act == ACT_SWIGLU_PAIR || g.act == ACT_ROPE_QK) return true;   // the paired epilogues exist in the 256x256 kernel only
  if (batch > 8) return false;                        // its flat work decode walks at most 8 batches
  if (mp_gemm_variant() != 2) return false;
  const int64_t tiles = mp_cdiv(g.M, 256) * mp_cdiv(g.N, 256) * batch;
  static int min_tiles = -1, min_n = -1;
  if (min_tiles < 0) {
    const char* e = getenv("MP_GEMM256_MIN_TILES");
    min_tiles = (e && atoi(e) >= 1) ? atoi(e) : 128;
    const char* f = getenv("MP_GEMM256_MIN_N");
    min_n = (f && atoi(f) >= 1) ? atoi(f) : 1024;
  }
  // short K with a small second tile wave (CLIP fc1 / mm_projector.0: 304 / 288 tiles, 16 K-tiles): the tail split leaves 4-K-tile
  // units that are all prologue and epilogue; the 128x128 kernel measured 67 vs 79 us there
  static int shortk = -1;
  if (shortk < 0) { const char* e = getenv("MP_GEMM_SHORTK_RULE"); shortk = (e && atoi(e) == 0) ? 0 : 1; }
  if (shortk && g.K <= 1024 && tiles > 256 && (tiles % 256) > 0 && (tiles % 256) < 128) return false;
  // few tiles but a long K (CLIP fc2: 4616 x 1024 x 4096 = 76 tiles): the tail split cuts each tile into K-ranges of >= 16 K-tiles that
  // fill the machine (3 x 76 units): 64 vs 77 us on the 128x128 kernel (scripts/tower_ab.sh)
  if (g.M >= 1024 && g.N >= min_n && tiles >= 64 && tiles < min_tiles && g.K >= 4096 && !g.m_dev && !g.out_f32) return true;
  return g.M >= 1024 && g.N >= min_n && tiles >= min_tiles;
}

// what the RoPE epilogue of the 320-row kernel costs on top of the plain one, in microseconds per wave of tiles (see gemm320_bf16.hip)
#define MP_GEMM320_ROPE_EXTRA_US 6.0

// The tile mode both 320-row rules start from: this thread's mp_gemm_tile_policy(), else MP_GEMM320 (0 never, 2 whenever eligible, default 1 = by the
// rule of the call's route).
static thread_local int g_tile_policy = -1;          // mp_gemm_tile_policy(): -1 = the process default (MP_GEMM320, else 1)
static int tile_mode() {
  static int env_mode = -1;
  if (env_mode < 0) { const char* e = getenv("MP_GEMM320"); env_mode = (e && e[0] >= '0' && e[0] <= '2') ? e[0] - '0' : 1; }
  return g_tile_policy >= 0 ? g_tile_policy : env_mode;
}

// 320-row tiles, or the kernel the call would otherwise get?  Modelled time in microseconds, from K sweeps at one full wave of tiles
// (scripts/gemm_ksweep.py, same box): a wave of 256x256 tiles costs 8.5 + 1.45 per 64-deep K step (prologue + epilogue, then 1480-1530
// TFLOP/s in the loop), a wave of 320x256 tiles 4.5 + 1.685 per step (1590-1640 TFLOP/s in the loop; the fixed part was 30 us until the
// kernel was split by epilogue family, see gemm320_bf16.hip); a residual epilogue adds ~8 to either, QuickGELU ~6.  The 256 tiling pays
// floor(T / C) whole waves plus a tail (a whole wave when more than half the CUs have a tile, else 1 / S of one for the S-way split
// plus ~0.3 for the partials' round trip through memory); the 320 tiling has no tail split: all its waves are whole.  Where the 256x256
// rule does not apply (short K with a small second wave, narrow N) the alternative is the 128x128 kernel at the ~560 TFLOP/s it reaches
// on such shapes (CLIP fc1: 72 us against 43.5 on 320-row tiles).  MP_GEMM320 = 0 never, 2 whenever eligible, default 1 = by this model.
static bool use_320(const GemmArgs& g, int batch, hipStream_t stream) {
  const int mode = tile_mode();
  if (mode == 0 || mp_gemm_variant() != 2 || !mp_gemm320_eligible(g, batch)) return false;
  if (mode >= 2) return true;
  const int C = std::min(mp_device_cus(), 256);
  const int64_t t256 = mp_cdiv(g.M, 256) * mp_cdiv(g.N, 256), t320 = mp_cdiv(g.M, 320) * (g.N / 256);
  if (t320 * 2 < C && (mp_gemm_stream_registered(stream) || mp_gemm320_subwave_split(g, batch) <= 1)) return false;   // fewer workgroups than half the CUs: the smaller tiles (or a K split) fill the machine better
  const double k = g.K / 64.0;
  const double epi = (g.residual ? 8.0 : 0.0) + (g.act == ACT_QUICK_GELU ? 6.0 : 0.0);
  const double rope320 = g.act == ACT_ROPE_QK ? MP_GEMM320_ROPE_EXTRA_US : 0.0;
  const double w320 = (double)mp_cdiv(t320, C);          // dense calls run whole waves (the kernel's tail split is for the batched expert calls)
  double c320 = w320 * (4.5 + epi + rope320 + 1.685 * k);
  // at most half a wave of tiles and a long K: every tile cut S ways with the cooperative fix-up (mp_gemm320_subwave_split; the primary stream only,
  // like every split).  MP_GEMM320_SUBWAVE_FIX_US: the fix-up's price in the model (partials written and read back: ~2 x 84 MB at S = 2)
  if (!mp_gemm_stream_registered(stream)) {
    const int S = mp_gemm320_subwave_split(g, batch);
    if (S > 1) {
      static double fix_us = -1.0;
      if (fix_us < 0) { const char* e = getenv("MP_GEMM320_SUBWAVE_FIX_US"); fix_us = (e && atof(e) > 0) ? atof(e) : 28.0; }
      c320 = std::min(c320, 4.5 + epi + 1.685 * k / S + fix_us);
    }
  }
  double other;
  if (use_256_rule(g, batch)) {
    const int64_t rem = t256 % C;
    double w256 = (double)(t256 / C);
    if (rem > 0) {
      const int S = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(C / rem, 8), g.K / 64 / 4));
      w256 += (rem * 2 > C || S == 1) ? 1.0 : 1.0 / S + 0.3;
    }
    other = w256 * (8.5 + epi + 1.45 * k);
  } else {
    other = 2.0 * g.M * g.N * g.K / 560e6;
  }
  return c320 < 0.98 * other;
}

// Batched calls (the MoE expert projections: per-expert device-side row counts, rows gathered / scattered through the routing tables).  The
// host does not know the row counts, so there is no wave model here: the 320-row tiles take the eligible calls with a long K and N >= 8192
// (gate|up: N = 22016, K = 4096: 86 column tiles, so a row tile more or less moves the wave count by a few percent) -- their K loop runs
// ~5 % faster and a wave of tiles costs 4 us less in prologue and epilogue than a wave of 256x256 tiles: 665-677 us against 722-787 for
// E = 2 at 5112 tokens (scripts/expert_gemm_ab.py).  The down projection (N = 4096: 16 column tiles) stays on 256x256 tiles: 2556 + 2556
// rows are 8 + 8 row tiles of 320 = exactly one wave (308 us against 365), but 2500 + 2612 are 8 + 9 = 1.06 waves and this kernel had no
// tail split then (531 us against 380); with the tail split the kernel has since got (16 tiles cut 8 ways) it measures 375-381 against
// 380-383: the routing is never balanced to the row, so there is nothing to win and the rule stays N >= 8192.  MP_GEMM320_BATCHED=0: never (A/B).
static bool use_320_batched(const GemmArgs& g, int batch) {
  static int env_b = -1;
  if (env_b < 0) { const char* e = getenv("MP_GEMM320_BATCHED"); env_b = (e && atoi(e) == 0) ? 0 : 1; }
  const int mode = tile_mode();
  if (mode == 0 || mp_gemm_variant() != 2 || !mp_gemm320_eligible(g, batch)) return false;
  if (mode >= 2) return true;
  if (!env_b) return false;
  if (g.K >= 2048 && g.N >= 8192) return true;
  // round 3: the experts' down projection (N = 4096, K = 11008, combine epilogue) too.  8 + 9 row tiles of 320 are 272 tiles = one wave
  // + 16 tail tiles; the tail is now cut 10 ways with a COOPERATIVE fix-up (every unit reduces and stores a share of the tile instead
  // of the last arriver summing S x 320 KiB alone, gemm320_bf16.hip), which is what the rule above was waiting for.  MP_GEMM320_DOWN=0: A/B.
  static int env_d = -1;
  if (env_d < 0) { const char* e = getenv("MP_GEMM320_DOWN"); env_d = (e && atoi(e) == 0) ? 0 : 1; }
  return env_d && g.c_rows && g.K >= 8192 && g.N >= 2048;
}

// which kernel the last bf16 GEMM entry of this thread dispatched to (bench.py attributes its HIP-event samples per kernel)
static thread_local int g_last_gemm_kernel = 0;
extern "C" int mp_gemm_last_kernel(void) { return g_last_gemm_kernel; }
// policy 3 (the frozen towers): the 320-row kernel's tails never split, whichever stream the call is on (gemm320_bf16.hip: mp_launch_gemm320)
bool mp_gemm_policy_whole_tiles() { return g_tile_policy == 3; }
// mp_gemm_tail_wait(): how long (shader cycles) a unit of the 320-row kernel's split tail waits for its siblings before the tile falls
// back to "the last unit finishes alone".  Default 150 k cycles (~60-80 us: several K-ranges of the longest split the decoder runs);
// 0 = never wait (every tile decides at once: the test of the fallback path), MP_GEMM320_TAIL_WAIT overrides the default.
static long long g_tail_wait = -1;
long long mp_gemm_tail_wait_value() {
  if (g_tail_wait < 0) { const char* e = getenv("MP_GEMM320_TAIL_WAIT"); g_tail_wait = (e && atoll(e) >= 0) ? atoll(e) : 150000; }
  return g_tail_wait;
}
extern "C" int64_t mp_gemm_tail_wait(int64_t cycles) {
  const long long prev = mp_gemm_tail_wait_value();
  if (cycles >= 0) g_tail_wait = cycles;
  return prev;
}
extern "C" int mp_gemm_tile_policy(int mode) {
  MP_REQUIRE(mode >= -1 && mode <= 3, MP_ERR_ARG, "mp_gemm_tile_policy: mode must be -1 (default), 0 (256-row tiles only), 1 (by the wave model), 2 (320-row tiles whenever eligible) or 3 (as 2, tails never split)");
  g_tile_policy = mode;
  return MP_OK;
}

// One call, one kernel.  The route names the rule that may give the call the 320-row tiles: the wave model (dense calls), the batched rule (the MoE
// expert calls), or no choice at all (the folded-norm entries, whose epilogue only the 320-row kernel has).  What the 320-row tiles do not take goes
// to the 256x256 kernel by use_256_rule() and to the 128x128 kernel otherwise.  `name` = the entry point, for messages and the 128x128 launch check.
enum Route { ROUTE_DENSE, ROUTE_BATCHED, ROUTE_DENSE_320_ONLY, ROUTE_BATCHED_320_ONLY };

static int dispatch_gemm(const GemmArgs& g, int batch, hipStream_t stream, Route route, const char* name) {
  bool big;
  switch (route) {
    case ROUTE_DENSE: big = use_320(g, batch, stream); break;
    case ROUTE_BATCHED: big = use_320_batched(g, batch); break;
    case ROUTE_DENSE_320_ONLY:
      MP_REQUIRE(mp_gemm_variant() == 2 && mp_gemm320_eligible(g, batch), MP_ERR_SHAPE,
                 "%s: M=%d N=%d K=%d is not a 320-row-kernel shape (M >= 1024, N %% 256 == 0)", name, g.M, g.N, g.K);
      big = true;
      break;
    case ROUTE_BATCHED_320_ONLY:
      MP_REQUIRE(mp_gemm_variant() == 2 && mp_gemm320_eligible(g, batch), MP_ERR_SHAPE,
                 "%s: M=%d N=%d K=%d batch=%d is not a 320-row-kernel shape (M >= 1024, N %% 256 == 0)", name, g.M, g.N, g.K, batch);
      big = true;
      break;
    default:
      MP_REQUIRE(false, MP_ERR_ARG, "%s: unknown GEMM route %d", name, (int)route);
  }
  if (big) { g_last_gemm_kernel = 320; return mp_launch_gemm320(g, batch, stream); }
  const bool mid = use_256_rule(g, batch);
  g_last_gemm_kernel = mid ? 256 : 128;
  if (mid) return mp_launch_gemm256(g, batch, stream);
  mp_launch_gemm128(g, batch, /*may_split=*/route == ROUTE_DENSE, stream);     // the batched launches never split: one accumulation order per expert
  return mp_check_launch(name);
}

// what every entry point passes on as it got it; the rest of the block stays zero (no bias, residual, batching, gather ...) until the entry sets it
static GemmArgs gemm_args(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, int M, int N, int K, int act, int out_dtype) {
  GemmArgs g{};
  g.A = (const bf16_t*)A; g.lda = lda; g.W = (const bf16_t*)W; g.ldw = ldw; g.C = C; g.ldc = ldc;
  g.M = M; g.N = N; g.K = K; g.act = act; g.out_f32 = (out_dtype == MP_F32); g.alpha = 1.f; g.group_m = gemm_group_m();
  return g;
}

// C-ABI: see include/medplib_hip.h
extern "C" int mp_gemm_bf16_nt(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc,
                               const float* bias, const void* residual, int64_t ldr, int M, int N, int K, int act,
                               int out_dtype, float alpha, const int* m_dev, hipStream_t stream) {
  MP_REQUIRE(M >= 0 && N > 0 && K > 0, MP_ERR_SHAPE, "mp_gemm_bf16_nt: bad shape M=%d N=%d K=%d", M, N, K);
  MP_REQUIRE(K % BK == 0, MP_ERR_SHAPE, "mp_gemm_bf16_nt: K=%d must be a multiple of %d (pad on the host)", K, BK);
  MP_REQUIRE(lda % 8 == 0 && ldw % 8 == 0, MP_ERR_SHAPE, "mp_gemm_bf16_nt: lda/ldw must be multiples of 8");
  MP_REQUIRE(out_dtype == MP_BF16 || out_dtype == MP_F32, MP_ERR_DTYPE, "mp_gemm_bf16_nt: bad out dtype %d", out_dtype);
  MP_REQUIRE(act >= 0 && act <= 5, MP_ERR_ARG, "mp_gemm_bf16_nt: bad activation %d", act);
  MP_REQUIRE(act != ACT_SWIGLU_PAIR || (N % 64 == 0 && out_dtype == MP_BF16 && residual == nullptr && ldc % 8 == 0), MP_ERR_ARG,
             "mp_gemm_bf16_nt: SWIGLU_PAIR needs N %% 64 == 0, bf16 output [M, N/2] with ldc %% 8 == 0 and no residual");
  if (M == 0) return MP_OK;
  GemmArgs g = gemm_args(A, lda, W, ldw, C, ldc, M, N, K, act, out_dtype);
  g.bias = bias; g.residual = (const bf16_t*)residual; g.ldr = ldr; g.m_dev = m_dev; g.alpha = alpha;
  return dispatch_gemm(g, 1, stream, ROUTE_DENSE, "mp_gemm_bf16_nt");
}

// Fused qkv projection + RoPE (LlamaAttention: q_proj / k_proj / v_proj + apply_rotary_pos_emb): C[M, 3*hidden] =
// A[M, K] @ Wi[3*hidden, K]^T with the rotation of the q and k thirds done in the epilogue.  Wi = the fused qkv weight with the rows
// of every q / k head interleaved in blocks of 32 (ACT_ROPE_QK, gemm_common.h); C comes out in the standard layout.
extern "C" int mp_gemm_qkv_rope_bf16(const void* A, int64_t lda, const void* Wi, int64_t ldw, void* C, int64_t ldc, const float* cos_t,
                                     const float* sin_t, int M, int N, int K, int seq, int pos_offset, int head_dim, hipStream_t stream) {
  MP_REQUIRE(M >= 0 && N > 0 && K > 0 && K % BK == 0, MP_ERR_SHAPE, "mp_gemm_qkv_rope_bf16: K must be a multiple of %d", BK);
  MP_REQUIRE(head_dim == 128 && N % 3 == 0 && (N / 3) % 256 == 0, MP_ERR_SHAPE,
             "mp_gemm_qkv_rope_bf16: head_dim 128 and hidden %% 256 == 0 (got head_dim %d, N %d)", head_dim, N);
  MP_REQUIRE(lda % 8 == 0 && ldw % 8 == 0 && ldc % 4 == 0 && cos_t && sin_t && seq > 0, MP_ERR_ARG, "mp_gemm_qkv_rope_bf16: bad arguments");
  if (M == 0) return MP_OK;
  GemmArgs g = gemm_args(A, lda, Wi, ldw, C, ldc, M, N, K, ACT_ROPE_QK, MP_BF16);
  g.rope_cos = cos_t; g.rope_sin = sin_t; g.rope_seq = seq; g.rope_pos0 = pos_offset;
  return dispatch_gemm(g, 1, stream, ROUTE_DENSE, "mp_gemm_qkv_rope_bf16");
}

// The same with the input RMSNorm folded in (config.fold_input_norm): A = the RAW residual stream, Wi = the interleaved qkv weight with the norm
// weight multiplied into its columns, row_scale [M] = rstd of every row (mp_rmsnorm_gate_rstd_bf16 with n_experts = 0): the epilogue multiplies
// the fp32 accumulators by rstd before the projection's bf16 rounding and the rotation.  320-row kernel only: a shape it does not take is an error
// (the caller keeps the unfolded path for those).
extern "C" int mp_gemm_qkv_rope_scaled_bf16(const void* A, int64_t lda, const void* Wi, int64_t ldw, void* C, int64_t ldc, const float* cos_t,
                                            const float* sin_t, const float* row_scale, int M, int N, int K, int seq, int pos_offset, int head_dim,
                                            hipStream_t stream) {
  MP_REQUIRE(M >= 0 && N > 0 && K > 0 && K % BK == 0, MP_ERR_SHAPE, "mp_gemm_qkv_rope_scaled_bf16: K must be a multiple of %d", BK);
  MP_REQUIRE(head_dim == 128 && N % 3 == 0 && (N / 3) % 256 == 0, MP_ERR_SHAPE, "mp_gemm_qkv_rope_scaled_bf16: head_dim 128 and hidden %% 256 == 0");
  MP_REQUIRE(lda % 8 == 0 && ldw % 8 == 0 && ldc % 4 == 0 && cos_t && sin_t && row_scale && seq > 0, MP_ERR_ARG, "mp_gemm_qkv_rope_scaled_bf16: bad arguments");
  if (M == 0) return MP_OK;
  GemmArgs g = gemm_args(A, lda, Wi, ldw, C, ldc, M, N, K, ACT_ROPE_QK, MP_BF16);
  g.rope_cos = cos_t; g.rope_sin = sin_t; g.rope_seq = seq; g.rope_pos0 = pos_offset;
  g.a_scale = row_scale;
  return dispatch_gemm(g, 1, stream, ROUTE_DENSE_320_ONLY, "mp_gemm_qkv_rope_scaled_bf16");
}

// mp_gemm_qkv_rope_bf16 / _scaled_ with the RoPE table's row count known on the host: every position (row % seq) + pos_offset must
// have a row, otherwise MP_ERR_SHAPE before any launch
static int qkv_rope_bound_check(const char* name, const float* cos_t, const float* sin_t, int seq, int pos_offset, int table_rows) {
  MP_REQUIRE(cos_t && sin_t, MP_ERR_ARG, "%s: null RoPE table", name);
  MP_REQUIRE(pos_offset >= 0 && seq > 0 && (int64_t)seq + pos_offset <= table_rows, MP_ERR_SHAPE,
             "%s: positions up to seq + pos_offset = %lld need that many RoPE table rows (table_rows = %d)", name,
             (long long)seq + pos_offset, table_rows);
  return MP_OK;
}

extern "C" int mp_gemm_qkv_rope_bounded_bf16(const void* A, int64_t lda, const void* Wi, int64_t ldw, void* C, int64_t ldc,
                                             const float* cos_t, const float* sin_t, int M, int N, int K, int seq, int pos_offset,
                                             int head_dim, int table_rows, hipStream_t stream) {
  const int rc = qkv_rope_bound_check("mp_gemm_qkv_rope_bounded_bf16", cos_t, sin_t, seq, pos_offset, table_rows);
  if (rc != MP_OK) return rc;
  return mp_gemm_qkv_rope_bf16(A, lda, Wi, ldw, C, ldc, cos_t, sin_t, M, N, K, seq, pos_offset, head_dim, stream);
}

extern "C" int mp_gemm_qkv_rope_scaled_bounded_bf16(const void* A, int64_t lda, const void* Wi, int64_t ldw, void* C, int64_t ldc,
                                                    const float* cos_t, const float* sin_t, const float* row_scale, int M, int N, int K,
                                                    int seq, int pos_offset, int head_dim, int table_rows, hipStream_t stream) {
  const int rc = qkv_rope_bound_check("mp_gemm_qkv_rope_scaled_bounded_bf16", cos_t, sin_t, seq, pos_offset, table_rows);
  if (rc != MP_OK) return rc;
  return mp_gemm_qkv_rope_scaled_bf16(A, lda, Wi, ldw, C, ldc, cos_t, sin_t, row_scale, M, N, K, seq, pos_offset, head_dim, stream);
}

// gate|up projection of a TRAINING forward: act = silu(gate) * up from the fused epilogue AND the bf16 gate|up values themselves (the
// backward's operands), one launch instead of GEMM + mp_swiglu_pair_fwd_bf16 (which re-read the [tokens, 2 ff] tensor).
extern "C" int mp_gemm_swiglu_keep_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, void* act_out, int64_t ld_act, void* gu_out,
                                        int64_t ld_gu, int M, int N, int K, hipStream_t stream) {
  MP_REQUIRE(M >= 0 && N > 0 && K > 0 && K % BK == 0 && N % 64 == 0, MP_ERR_SHAPE, "mp_gemm_swiglu_keep_bf16: K %% %d == 0 and N %% 64 == 0", BK);
  MP_REQUIRE(lda % 8 == 0 && ldw % 8 == 0 && ld_act % 8 == 0 && ld_gu % 8 == 0 && act_out && gu_out &&
                 (reinterpret_cast<uintptr_t>(act_out) & 15) == 0 && (reinterpret_cast<uintptr_t>(gu_out) & 15) == 0,
             MP_ERR_ARG, "mp_gemm_swiglu_keep_bf16: strides must be multiples of 8, outputs 16-byte aligned");
  if (M == 0) return MP_OK;
  GemmArgs g = gemm_args(A, lda, W, ldw, act_out, ld_act, M, N, K, ACT_SWIGLU_PAIR, MP_BF16);
  g.keep_gu = (bf16_t*)gu_out; g.ld_gu = ld_gu;
  return dispatch_gemm(g, 1, stream, ROUTE_DENSE, "mp_gemm_swiglu_keep_bf16");
}

// batched variant: `batch` independent problems at fixed element strides (expert GEMMs: one launch over all experts,
// with per-expert device-side row counts m_dev[b]).
extern "C" int mp_gemm_bf16_nt_batched(const void* A, int64_t lda, int64_t strideA, const void* W, int64_t ldw,
                                       int64_t strideW, void* C, int64_t ldc, int64_t strideC, const float* bias,
                                       int64_t strideBias, int batch, int M, int N, int K, int act, int out_dtype,
                                       const int* m_dev, hipStream_t stream) {
  MP_REQUIRE(M >= 0 && N > 0 && K > 0 && batch > 0, MP_ERR_SHAPE, "mp_gemm_bf16_nt_batched: bad shape");
  MP_REQUIRE(K % BK == 0, MP_ERR_SHAPE, "mp_gemm_bf16_nt_batched: K=%d must be a multiple of %d", K, BK);
  MP_REQUIRE(lda % 8 == 0 && ldw % 8 == 0 && strideA % 8 == 0 && strideW % 8 == 0, MP_ERR_SHAPE,
             "mp_gemm_bf16_nt_batched: strides must be multiples of 8");
  MP_REQUIRE(out_dtype == MP_BF16 || out_dtype == MP_F32, MP_ERR_DTYPE, "mp_gemm_bf16_nt_batched: bad out dtype");
  MP_REQUIRE(act >= 0 && act <= 5, MP_ERR_ARG, "mp_gemm_bf16_nt_batched: bad activation %d", act);
  MP_REQUIRE(act != ACT_SWIGLU_PAIR || (N % 64 == 0 && out_dtype == MP_BF16 && ldc % 8 == 0), MP_ERR_ARG,
             "mp_gemm_bf16_nt_batched: SWIGLU_PAIR needs N %% 64 == 0 and a bf16 [M, N/2] output");
  if (M == 0) return MP_OK;
  GemmArgs g = gemm_args(A, lda, W, ldw, C, ldc, M, N, K, act, out_dtype);
  g.bias = bias; g.m_dev = m_dev; g.m_dev_stride = 1;
  g.sA = strideA; g.sW = strideW; g.sC = strideC; g.sBias = strideBias;
  return dispatch_gemm(g, batch, stream, ROUTE_BATCHED, "mp_gemm_bf16_nt_batched");
}

// batched variant with a batched residual: C[b] = bf16(A[b] W[b]^T) + R[b] (the per-expert LoRA delta added onto the expert projection's
// output in training, llama_lora.py)
extern "C" int mp_gemm_bf16_nt_batched_res(const void* A, int64_t lda, int64_t strideA, const void* W, int64_t ldw, int64_t strideW, void* C,
                                           int64_t ldc, int64_t strideC, const void* residual, int64_t ldr, int64_t strideR, int batch, int M,
                                           int N, int K, const int* m_dev, hipStream_t stream) {
  MP_REQUIRE(M >= 0 && N > 0 && K > 0 && batch > 0 && K % BK == 0, MP_ERR_SHAPE, "mp_gemm_bf16_nt_batched_res: bad shape");
  MP_REQUIRE(lda % 8 == 0 && ldw % 8 == 0 && strideA % 8 == 0 && strideW % 8 == 0 && residual, MP_ERR_SHAPE,
             "mp_gemm_bf16_nt_batched_res: strides must be multiples of 8, residual required");
  if (M == 0) return MP_OK;
  GemmArgs g = gemm_args(A, lda, W, ldw, C, ldc, M, N, K, ACT_NONE, MP_BF16);
  g.residual = (const bf16_t*)residual; g.ldr = ldr; g.m_dev = m_dev; g.m_dev_stride = 1;
  g.sA = strideA; g.sW = strideW; g.sC = strideC; g.sR = strideR;
  return dispatch_gemm(g, batch, stream, ROUTE_BATCHED, "mp_gemm_bf16_nt_batched_res");
}

// Expert GEMMs with the MoE dispatch / combine folded in (top-1 routing): per expert b, A row r comes from row a_rows[b*rows_stride+r]
// of the shared [tokens, K] activation matrix (a_rows null = A is [batch, M, K] as in the plain batched call), and — when c_rows is
// given — C row r goes to row c_rows[b*rows_stride+r] of the shared [tokens, N] output as residual[row] + c_scale[row] * bf16(acc).
extern "C" int mp_gemm_bf16_nt_batched_rows(const void* A, int64_t lda, int64_t strideA, const int* a_rows, const void* W, int64_t ldw,
                                            int64_t strideW, void* C, int64_t ldc, int64_t strideC, const int* c_rows,
                                            const float* c_scale, const void* residual, int64_t ldr, int rows_stride, int batch, int M,
                                            int N, int K, int act, const int* m_dev, hipStream_t stream) {
  MP_REQUIRE(M >= 0 && N > 0 && K > 0 && batch > 0, MP_ERR_SHAPE, "mp_gemm_bf16_nt_batched_rows: bad shape");
  MP_REQUIRE(K % BK == 0 && lda % 8 == 0 && ldw % 8 == 0 && strideW % 8 == 0, MP_ERR_SHAPE, "mp_gemm_bf16_nt_batched_rows: K %% 64, strides %% 8");
  MP_REQUIRE(act == ACT_NONE || act == ACT_SWIGLU_PAIR, MP_ERR_ARG, "mp_gemm_bf16_nt_batched_rows: activation must be none or SWIGLU_PAIR");
  MP_REQUIRE(act != ACT_SWIGLU_PAIR || (N % 64 == 0 && ldc % 8 == 0 && !c_rows), MP_ERR_ARG, "mp_gemm_bf16_nt_batched_rows: bad SWIGLU_PAIR use");
  MP_REQUIRE(!c_rows || (N % 4 == 0 && ldc % 4 == 0 && (!residual || ldr % 4 == 0)), MP_ERR_SHAPE, "mp_gemm_bf16_nt_batched_rows: scatter needs N, ldc, ldr %% 4 == 0");
  MP_REQUIRE(c_rows || (!c_scale && !residual), MP_ERR_ARG, "mp_gemm_bf16_nt_batched_rows: c_scale / residual come with c_rows");
  if (M == 0) return MP_OK;
  GemmArgs g = gemm_args(A, lda, W, ldw, C, ldc, M, N, K, act, MP_BF16);
  g.residual = (const bf16_t*)residual; g.ldr = ldr; g.m_dev = m_dev; g.m_dev_stride = 1;
  g.sA = a_rows ? 0 : strideA; g.sW = strideW; g.sC = c_rows ? 0 : strideC;
  g.a_rows = a_rows; g.c_rows = c_rows; g.c_scale = c_scale; g.rows_stride = rows_stride;
  return dispatch_gemm(g, batch, stream, ROUTE_BATCHED, "mp_gemm_bf16_nt_batched_rows");
}

// The expert gate|up projection with the post-attention RMSNorm folded in: A = the RAW residual stream [tokens, K] gathered through a_rows, W = the
// interleaved gate|up weights with the norm weight multiplied into their columns, a_row_scale [tokens] = rstd (mp_rmsnorm_gate_rstd_bf16).  The
// SwiGLU epilogue multiplies the fp32 accumulators by rstd[token of the row] before their bf16 rounding.  SWIGLU_PAIR, 320-row kernel only.
extern "C" int mp_gemm_bf16_nt_batched_rows_scaled(const void* A, int64_t lda, const int* a_rows, const float* a_row_scale, const void* W, int64_t ldw,
                                                   int64_t strideW, void* C, int64_t ldc, int64_t strideC, int rows_stride, int batch, int M, int N,
                                                   int K, const int* m_dev, hipStream_t stream) {
  MP_REQUIRE(M >= 0 && N > 0 && K > 0 && batch > 0 && a_rows && a_row_scale, MP_ERR_ARG, "mp_gemm_bf16_nt_batched_rows_scaled: a_rows and a_row_scale required");
  MP_REQUIRE(K % BK == 0 && lda % 8 == 0 && ldw % 8 == 0 && strideW % 8 == 0 && N % 64 == 0 && ldc % 8 == 0, MP_ERR_SHAPE, "mp_gemm_bf16_nt_batched_rows_scaled: bad strides");
  if (M == 0) return MP_OK;
  GemmArgs g = gemm_args(A, lda, W, ldw, C, ldc, M, N, K, ACT_SWIGLU_PAIR, MP_BF16);
  g.m_dev = m_dev; g.m_dev_stride = 1; g.sW = strideW; g.sC = strideC;
  g.a_rows = a_rows; g.rows_stride = rows_stride; g.a_scale = a_row_scale;
  return dispatch_gemm(g, batch, stream, ROUTE_BATCHED_320_ONLY, "mp_gemm_bf16_nt_batched_rows_scaled");
}

// Whether the two folded-norm GEMM entry points take a call of this size (the host keeps the unfolded path otherwise)
extern "C" int mp_gemm_fold_ok(int M, int N, int K) { return (mp_gemm_variant() == 2 && M >= 1024 && N % 256 == 0 && K % 64 == 0) ? 1 : 0; }
