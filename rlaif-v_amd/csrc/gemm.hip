// C-ABI launchers for the bf16 NT GEMM and the fused LM-head log-prob kernels (gemm.hpp).
#include "gemm.hpp"
#include "host.hpp"
#include "rlaifv_hip.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

static thread_local char g_err[512] = "";
void rv_set_error(const char* msg) {
  strncpy(g_err, msg ? msg : "", sizeof(g_err) - 1);
  g_err[sizeof(g_err) - 1] = 0;
}
void rv_set_errorf(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---- A/B knobs: each is read through one accessor, from the first call of any entry point on ----
// variants: 0 = 128x128x64 register staging, 1 = 128x128x64 global_load_lds, 2 = 256x256x32 ping-pong,
// -1 (default) = pick 2 when the problem fills the chip with 256x256 tiles, else 1.
static int g_default_variant = -1;
// RV_EPI_WIDE=0: the 4-wide EpiStore path
static int epi_narrow() {
  static const int v = env_int("RV_EPI_WIDE", 1) == 0 ? 1 : 0;
  return v;
}
// experiment knob RV_GEMM_GROUP: row tiles per scheduling group (GemmShape::group)
static int gemm_group() {
  static const int v = env_int("RV_GEMM_GROUP", 0);
  return v;
}
// RV_GEMM_MI16 (default 1): the 16x16x32-MFMA main loops of the 64-deep-A NN kernel and the TN kernel (gemm.hpp "MI16"); 0 = 32x32x16
static int g_mi16 = -1;
static int nn_mi16() {
  if (g_mi16 < 0) g_mi16 = env_int("RV_GEMM_MI16", 1);
  return g_mi16;
}

static int tiles(int n, int tile) { return (n + tile - 1) / tile; }
// the chip-fill rule of the 256x256 kernels (ops.py _fills_chip mirrors it)
static bool fills_chip(const GemmShape& g) { return (long)tiles(g.M, G2_BM) * tiles(g.N, G2_BN) >= 192; }

// ---- argument checks.  Every message names the entry point that was called. ----
#define REQ(cond, what) RV_REQUIRE_AS(who, cond, what)
#define CHECK(call)                             \
  do {                                          \
    if (call) return 1;                         \
  } while (0)

// leading dimensions, in elements: multiples of 8 where rows are moved 16 bytes at a time (every input, and the bf16 outputs of
// the rope and SwiGLU epilogues), multiples of 4 for the other outputs and the residuals
static int check_ld(const char* who, std::initializer_list<long> by8, std::initializer_list<long> by4) {
  for (long ld : by8) REQ(ld % 8 == 0, "a leading dimension of rows moved 16 bytes at a time must be a multiple of 8 elements");
  for (long ld : by4) REQ(ld % 4 == 0, "the leading dimension of an output or a residual must be a multiple of 4 elements");
  return 0;
}
static int check_align(const char* who, std::initializer_list<const void*> ptrs, int bytes, const char* names) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= (uintptr_t)p;
  if (bits & (uintptr_t)(bytes - 1)) {
    rv_set_errorf("%s: %s must be %d-byte aligned", who, names, bytes);
    return 1;
  }
  return 0;
}
// column groups of the second contraction segment: whole N tiles (128 for the NT kernels, 256 for the NN ones) that tile N
static int check_groups(const char* who, int group_cols, int group0, int N, int tile) {
  if (group_cols == 0 || (group_cols % tile == 0 && group0 % tile == 0 && group0 >= 0 && group0 <= N &&
                          (N - (group0 ? group0 : group_cols)) % group_cols == 0))
    return 0;
  rv_set_errorf("%s: group_cols / group0 must be multiples of %d that tile N (group0 + k * group_cols = N)", who, tile);
  return 1;
}
static int check_p(const char* who, float p) {
  REQ(p >= 0.f && p < 1.f, "0 <= p < 1");
  return 0;
}
// what the NT kernels ask of (A, B, N, K)
static int check_shape(const GemmShape& g, const char* who) {
  REQ(g.K % GEMM_BK == 0 && g.K > 0, "K must be a positive multiple of 64");
  REQ(g.N % 4 == 0, "N must be a multiple of 4");
  CHECK(check_ld(who, {g.lda, g.ldb}, {}));
  return check_align(who, {g.A, g.B}, 16, "A/B");
}

static GemmShape shape(const void* A, long lda, const void* B, long ldb, int M, int N, int K) {
  return GemmShape{(const bf16_t*)A, (const bf16_t*)B, M, N, K, lda, ldb, gemm_group()};
}
static GemmShape shape_ext(const void* A, long lda, const void* B, long ldb, int M, int N, int K, const void* A2, long lda2,
                           const void* B2, long ldb2, int K2, int group_cols, int group0) {
  return GemmShape{(const bf16_t*)A, (const bf16_t*)B, M, N, K, lda, ldb, gemm_group(),
                   (const bf16_t*)A2, (const bf16_t*)B2, lda2, ldb2, K2, group_cols, group0};
}
static EpiStore epi_store(void* C, long ldc, const void* bias, const void* residual, long ldr, int act, float alpha) {
  EpiStore epi{(bf16_t*)C, ldc, (const bf16_t*)bias, (const bf16_t*)residual, ldr, act, alpha};
  epi.narrow = epi_narrow();
  return epi;
}

// ---- NT launchers: 128x128 tiles (STAGE 0 = register staging, 1 = LDS-DMA) and 256x256 ping-pong; EXT = second K segment ----
template <int STAGE, class Epi, bool EXT = false>
static int launch_gemm(const GemmShape& g, const Epi& epi, void* st) {
  return launch<gemm_nt_kernel<STAGE, Epi, EXT>>(GEMM_LDS_BYTES, dim3(tiles(g.M, GEMM_BM) * tiles(g.N, GEMM_BN)), dim3(GEMM_THREADS),
                                                 st, g, epi);
}
template <class Epi, bool DMA_IN_MSEG, bool EXT = false>
static int launch_gemm256(const GemmShape& g, const Epi& epi, void* st) {
  return launch<gemm_nt_256_kernel<Epi, DMA_IN_MSEG, EXT>>(4 * G2_STAGE_BYTES, dim3(tiles(g.M, G2_BM) * tiles(g.N, G2_BN)),
                                                           dim3(G2_THREADS), st, g, epi);
}

template <class Epi>
static int dispatch(const char* who, const GemmShape& g, const Epi& epi, int variant, void* stream) {
  if (variant < 0) variant = g_default_variant;
  if (variant < 0) variant = fills_chip(g) ? 3 : 1;
  REQ(variant <= 3, "GEMM variant: 0..3");
  if (variant == 3) return launch_gemm256<Epi, true>(g, epi, stream);
  if (variant == 2) return launch_gemm256<Epi, false>(g, epi, stream);
  if (variant == 1) return launch_gemm<1, Epi>(g, epi, stream);
  return launch_gemm<0, Epi>(g, epi, stream);
}

// GEMMs with a second contraction segment (GemmShape::A2/B2/K2): the 256x256 ping-pong kernel when the problem
// fills the chip and the column groups are tile aligned, else the 128x128 kernel.
template <class Epi>
static int dispatch_ext(const GemmShape& g, const Epi& epi, void* stream) {
  if (fills_chip(g) && g.group_cols % G2_BN == 0 && g.group0 % G2_BN == 0)
    return launch_gemm256<Epi, true, true>(g, epi, stream);
  return launch_gemm<1, Epi, true>(g, epi, stream);
}

// ---- the NN launcher: the 64-deep-A kernel when K allows (K % 64 == 0, K >= 512; with EXT also K2 % 64 == 0), with the
// 16x16x32 main loop unless RV_GEMM_MI16=0, else the 32-deep kernel.  A64_ONLY: the entry point has required such a K, and the
// 32-deep kernel is not instantiated for its epilogue.  PRE (adapter segment first) exists in the 64-deep kernel only.
// (Any order of the three launches is correct.  This one - 32-deep, 64-deep, 64-deep MI16 - is the order the functions have had
// in .text, and the bytes of the TN kernels depend on where they lie: reordering shows up as four changed digests in
// kernel_resources.py --digest, see that tool's docstring.) ----
template <class Epi, bool EXT = false, bool PRE = false, bool A64_ONLY = PRE>
static int launch_nn(const GemmShape& g, const Epi& epi, void* st) {
  static_assert(A64_ONLY || !PRE, "the adapter-first form has no 32-deep kernel");
  const dim3 grid(tiles(g.M, G2_BM) * tiles(g.N, G2_BN)), block(G2_THREADS);
  [[maybe_unused]] const bool a64 = A64_ONLY || (g.K % 64 == 0 && g.K >= 512 && (!EXT || g.K2 % 64 == 0));
  if constexpr (!A64_ONLY) {
    if (!a64) return launch<gemm_nn_256_kernel<Epi, EXT>>(G2_LDS_BYTES, grid, block, st, g, epi);
  }
  if (!nn_mi16()) return launch<gemm_nn_a64_kernel<Epi, EXT, false, PRE>>(G4_LDS_BYTES, grid, block, st, g, epi);
  return launch<gemm_nn_a64_kernel<Epi, EXT, true, PRE>>(G4_LDS_BYTES, grid, block, st, g, epi);
}

// TN kernel: prefetch distance 3 (128 KiB LDS ring; distance 4 measured equal)
template <class Epi>
static int launch_gemm_tn(const bf16_t* P, long ldp, const bf16_t* Q, long ldq, int R, int I, int J, const Epi& epi,
                          void* st, int splits = 1, int r_chunk = 0, long split_stride = 0, int bid0 = 0,
                          int nblocks = 0) {
  constexpr int DIST = 3, LDS = (DIST + 1) * G2_STAGE_BYTES;
  const int gx = nblocks > 0 ? nblocks : tiles(I, 256) * tiles(J, 256);          // launch-order positions bid0 .. bid0 + gx - 1
  const dim3 grid(gx, splits), block(G2_THREADS);
  if (!nn_mi16())
    return launch<gemm_tn_256_kernel<Epi, DIST>>(LDS, grid, block, st, P, ldp, Q, ldq, R, I, J, epi, r_chunk, split_stride, gemm_group(),
                                                 bid0);
  return launch<gemm_tn_256_kernel<Epi, DIST, true>>(LDS, grid, block, st, P, ldp, Q, ldq, R, I, J, epi, r_chunk, split_stride,
                                                     gemm_group(), bid0);
}

// Token-axis split of a TN product: `splits` chunks of r_chunk rows (a multiple of 32), none of them empty
struct SplitK { int splits, r_chunk; };
static SplitK splitk_chunks(int R, int splits) {
  const int r_chunk = ((R + splits - 1) / splits + 31) / 32 * 32;
  return SplitK{(R + r_chunk - 1) / r_chunk, r_chunk};
}

// Tail split of a weight-gradient GEMM.  All output tiles cost the same (the contraction runs over every token), so a
// launch of T tiles takes ceil(T / 256) rounds on 256 CUs and the last round is as long as a full one however few tiles it
// holds (wgu: 1376 tiles = 5.375 rounds, wdown: 688 = 2.69).  (In practice a thin last round runs somewhat faster than a full
// one - fewer CUs share the fabric - so the measured gain is a third of this model's: wgu 3.76 -> 3.65 ms, step -0.5 %.)  Plan: the first floor(T / 256) * 256 launch-order positions
// run as they are; the `tail` remaining tiles are split s ways over the token axis (s x tail workgroups of 1 / s length,
// fp32 tile-dense slabs) and summed in fixed order by tn_tail_reduce_kernel.  The tail then takes ceil(tail * s / 256) / s of
// a round instead of 1.  s = 1: no split pays (or the problem has no full round).
struct TnTailPlan { int full_blocks, tail, splits, r_chunk; };
static TnTailPlan tn_tail_plan(int R, int I, int J) {
  const double penalty = 0.04;        // rounds charged per split for its fixed costs (prologue, slab store, reduce pass); measured:
                                      // 8 splits of the wgu tail gain nothing, 2 splits -2.7 % (profiles/r03_tn_tail_split.log)
  const int T = ((I + 255) / 256) * ((J + 255) / 256);
  TnTailPlan p{T, 0, 1, 0};
  const int full = T / 256, tail = T % 256;
  if (full < 1 || tail == 0) return p;
  double best = 1.0;
  int best_s = 1;
  const int cand[5] = {2, 3, 4, 6, 8};
  for (int c = 0; c < 5; ++c) {
    const int s = cand[c];
    if (R / s < 2048) break;                                   // keep every split a long contraction
    const double t = (double)((tail * s + 255) / 256) / s + penalty * s;
    if (t < best - 1e-9) { best = t; best_s = s; }
  }
  if (1.0 - best < 0.15) return p;                             // not worth two more launches
  p.full_blocks = full * 256;
  p.tail = tail;
  const SplitK s = splitk_chunks(R, best_s);
  p.splits = s.splits;
  p.r_chunk = s.r_chunk;
  return p;
}

// out tile = bf16(sum over splits of the fp32 slabs), fixed order; one workgroup per tail tile, same tile walk as the GEMM
__global__ __launch_bounds__(256) void tn_tail_reduce_kernel(const float* __restrict__ ws, int splits, int tail, int bid0, int I,
                                                              int J, int group, bf16_t* __restrict__ C, long ldc) {
  int i0, j0;
  tn_tile_origin((int)blockIdx.x + bid0, I, J, group, i0, j0);
  const float* base = ws + (long)blockIdx.x * 65536;
  for (int q = threadIdx.x; q < 256 * 64; q += 256) {          // 256 rows x 64 float4
    const int r = q >> 6, c4 = (q & 63) * 4;
    if (i0 + r >= I || j0 + c4 >= J) continue;
    float4 a = *(const float4*)(base + r * 256 + c4);
    for (int s = 1; s < splits; ++s) {
      const float4 b = *(const float4*)(base + (long)s * tail * 65536 + r * 256 + c4);
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    uint2 o;
    o.x = pack2bf(a.x, a.y);
    o.y = pack2bf(a.z, a.w);
    *(uint2*)(C + (long)(i0 + r) * ldc + j0 + c4) = o;
  }
}

// out[i][j] = bf16(alpha * sum_s ws[s][i][j])   (deterministic second pass of the split-K TN GEMM)
__global__ void splitk_reduce_kernel(const float* __restrict__ ws, int splits, int I, int J, float alpha,
                                     bf16_t* __restrict__ out, long ldc) {
  const long n4 = (long)I * J / 4;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += (long)gridDim.x * blockDim.x) {
    const long e = q * 4;
    float4 a = *(const float4*)(ws + e);
    for (int s = 1; s < splits; ++s) {
      const float4 b = *(const float4*)(ws + (long)s * I * J + e);
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    const long i = e / J, j = e % J;
    uint2 o;
    o.x = pack2bf(a.x * alpha, a.y * alpha);
    o.y = pack2bf(a.z * alpha, a.w * alpha);
    *(uint2*)(out + i * ldc + j) = o;
  }
}
static int launch_splitk_reduce(const float* ws, int splits, int I, int J, float alpha, void* out, long ldc, void* st) {
  const long blocks = ((long)I * J / 4 + 255) / 256;
  return launch<splitk_reduce_kernel>(0, dim3((int)(blocks < 2048 ? blocks : 2048)), dim3(256), st, ws, splits, I, J, alpha, (bf16_t*)out,
                                      ldc);
}

// ---- LoRA adapter dropout with one mask per peft module (kernels: gemm.hpp "ONE MASK PER peft MODULE") ----
static LoraMasks lora_masks(float p, int seed0, int seed1, int seed2) {
  const DropParams d = drop_params(p, seed0);                 // threshold and 1 / (1 - p) are the same for every module
  LoraMasks dm;
  dm.thresh16 = d.thresh16;
  dm.inv_keep = d.inv_keep;
  dm.key[0] = d.key;
  dm.key[1] = drop_params(p, seed1).key;
  dm.key[2] = drop_params(p, seed2).key;
  return dm;
}

// f(std::integral_constant<int, G>{}) for the G = FIRST .. 3 modules of a fused projection
template <int FIRST = 1, class F>
static int for_modules(int G, F&& f) {
  if constexpr (FIRST <= 1) {
    if (G == 1) return f(std::integral_constant<int, 1>{});
  }
  if (G == 2) return f(std::integral_constant<int, 2>{});
  return f(std::integral_constant<int, 3>{});
}

extern "C" {

const char* rv_last_error(void) { return g_err; }

int rv_set_gemm_variant(int variant) {
  RV_REQUIRE(variant >= -1 && variant <= 3, "rv_set_gemm_variant: -1 (auto), 0..3");
  g_default_variant = variant;
  return 0;
}

int rv_abi_version(void) { return RV_ABI_VERSION; }

int rv_set_gemm_mi16(int on) {
  g_mi16 = on ? 1 : 0;
  return 0;
}

int rv_gemm_nt_bf16(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K,
                    const void* bias, const void* residual, long ldr, int act, float alpha, int variant,
                    void* stream) {
  const char* const who = __func__;
  if (M == 0 || N == 0) return 0;
  const GemmShape g = shape(A, lda, B, ldb, M, N, K);
  CHECK(check_shape(g, who));
  CHECK(check_ld(who, {}, {ldc, residual ? ldr : 0}));
  // many rows, at most 256 columns, plain store: the streaming kernel (the rank-r side of LoRA)
  if (variant < 0 && g_default_variant < 0 && N % GSK_BN == 0 && N <= 256 && M >= 4096 && bias == nullptr &&
      residual == nullptr && act == RV_ACT_NONE && ((uintptr_t)C & 7) == 0)
    return launch<gemm_nt_skinny_kernel>(GSK_LDS_BYTES, dim3(tiles(M, GSK_BM) * (N / GSK_BN)), dim3(256), stream, g,
                                         (bf16_t*)C, ldc, alpha);
  return dispatch(who, g, epi_store(C, ldc, bias, residual, ldr, act, alpha), variant, stream);
}

// what the TN entries share: R > 0, an [I, J] output of whole 8-element pieces
static int check_tn(const char* who, int R, int I, int J) {
  REQ(R > 0, "R must be > 0");
  REQ(I % 8 == 0 && J % 8 == 0 && I >= 8 && J >= 8, "I and J must be multiples of 8");
  return 0;
}

int rv_gemm_tn_bf16(const void* P, long ldp, const void* Q, long ldq, void* C, long ldc, int R, int I, int J,
                    const void* residual, long ldr, float alpha, void* stream) {
  const char* const who = __func__;
  if (I == 0 || J == 0) return 0;
  CHECK(check_tn(who, R, I, J));
  CHECK(check_ld(who, {ldp, ldq}, {ldc, residual ? ldr : 0}));
  CHECK(check_align(who, {P, Q}, 16, "P/Q"));
  return launch_gemm_tn((const bf16_t*)P, ldp, (const bf16_t*)Q, ldq, R, I, J, epi_store(C, ldc, nullptr, residual, ldr, RV_ACT_NONE, alpha),
                        stream);
}

int rv_gemm_tn_workspace_floats(int R, int I, int J) {
  if (R <= 0 || I <= 0 || J <= 0) return 0;
  const TnTailPlan p = tn_tail_plan(R, I, J);
  return p.splits > 1 ? p.splits * p.tail * 65536 : 0;
}

int rv_gemm_tn_bf16_ws(const void* P, long ldp, const void* Q, long ldq, void* C, long ldc, int R, int I, int J,
                       float* workspace, long workspace_floats, void* stream) {
  const char* const who = __func__;
  if (I == 0 || J == 0) return 0;
  CHECK(check_tn(who, R, I, J));
  CHECK(check_ld(who, {ldp, ldq}, {ldc}));
  CHECK(check_align(who, {P, Q, workspace}, 16, "P/Q/workspace"));
  CHECK(check_align(who, {C}, 8, "C (the tail reduce stores 4 bf16 at a time)"));
  const bf16_t *p_ = (const bf16_t*)P, *q_ = (const bf16_t*)Q;
  const TnTailPlan p = tn_tail_plan(R, I, J);
  const EpiStore epi = epi_store(C, ldc, nullptr, nullptr, 0, RV_ACT_NONE, 1.0f);
  if (p.splits <= 1 || workspace == nullptr || workspace_floats < (long)p.splits * p.tail * 65536)
    return launch_gemm_tn(p_, ldp, q_, ldq, R, I, J, epi, stream);
  if (launch_gemm_tn(p_, ldp, q_, ldq, R, I, J, epi, stream, 1, 0, 0, 0, p.full_blocks)) return 1;
  if (launch_gemm_tn(p_, ldp, q_, ldq, R, I, J, EpiStoreF32{workspace, 256}, stream, p.splits, p.r_chunk, -1, p.full_blocks, p.tail)) return 1;
  return launch<tn_tail_reduce_kernel>(0, dim3(p.tail), dim3(256), stream, (const float*)workspace, p.splits, p.tail, p.full_blocks, I, J,
                                       gemm_group(), (bf16_t*)C, ldc);
}

int rv_gemm_nt_lora_bf16(const void* A, long lda, const void* B, long ldb, const void* A2, long lda2, const void* B2,
                         long ldb2, int K2, int group_cols, int group0, void* C, long ldc, int M, int N, int K,
                         const void* residual, long ldr, void* stream) {
  const char* const who = __func__;
  if (M == 0 || N == 0) return 0;
  const GemmShape g = shape_ext(A, lda, B, ldb, M, N, K, A2, lda2, B2, ldb2, K2, group_cols, group0);
  CHECK(check_shape(g, who));
  REQ(K2 > 0 && K2 % GEMM_BK == 0, "K2 must be a positive multiple of 64");
  CHECK(check_ld(who, {lda2, ldb2}, {ldc, residual ? ldr : 0}));
  CHECK(check_align(who, {A2, B2}, 16, "A2/B2"));
  CHECK(check_groups(who, group_cols, group0, N, GEMM_BN));
  return dispatch_ext(g, epi_store(C, ldc, nullptr, residual, ldr, RV_ACT_NONE, 1.0f), stream);
}

// rv_gemm_nn_bf16 and rv_gemm_nn_bias_act_bf16
static int nn_bias_act(const char* who, const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K,
                       const void* bias, const void* residual, long ldr, int act, float alpha, void* stream) {
  if (M == 0 || N == 0) return 0;
  REQ(K > 0 && K % G2_BK == 0, "K must be a positive multiple of 32");
  REQ(N % 8 == 0 && N >= 8, "N must be a multiple of 8");
  CHECK(check_ld(who, {lda, ldb}, {ldc, residual ? ldr : 0}));
  CHECK(check_align(who, {A, B}, 16, "A/B"));
  return launch_nn(shape(A, lda, B, ldb, M, N, K), epi_store(C, ldc, bias, residual, ldr, act, alpha), stream);
}

int rv_gemm_nn_bf16(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K,
                    const void* residual, long ldr, float alpha, void* stream) {
  return nn_bias_act(__func__, A, lda, B, ldb, C, ldc, M, N, K, nullptr, residual, ldr, RV_ACT_NONE, alpha, stream);
}

int rv_gemm_nn_bias_act_bf16(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K,
                             const void* bias, const void* residual, long ldr, int act, float alpha, void* stream) {
  const char* const who = __func__;
  REQ(act == RV_ACT_NONE || act == RV_ACT_QUICK_GELU || act == RV_ACT_GELU, "unknown activation");
  CHECK(check_align(who, {bias}, 16, "bias"));
  return nn_bias_act(who, A, lda, B, ldb, C, ldc, M, N, K, bias, residual, ldr, act, alpha, stream);
}

int rv_gemm_nn_rope_bf16(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K,
                         const float* cos_tab, const float* sin_tab, const int* pos, int L, int rope_cols, int hd, void* stream) {
  const char* const who = __func__;
  if (M == 0 || N == 0) return 0;
  REQ(hd == 128, "hd must be 128");
  REQ(K >= 512 && K % 64 == 0, "K must be a multiple of 64 and >= 512 (64-deep-A kernel)");
  REQ(N % 256 == 0 && rope_cols % 256 == 0 && rope_cols >= 0 && rope_cols <= N,
      "N and rope_cols must be multiples of 256 (a 256-column tile holds q / k heads or v heads)");
  CHECK(check_ld(who, {lda, ldb, ldc}, {}));
  CHECK(check_align(who, {A, B, C, cos_tab, sin_tab}, 16, "operands and tables"));
  REQ(cos_tab && sin_tab && L > 0, "cos_tab, sin_tab and L > 0 required");
  const EpiStoreRope epi{(bf16_t*)C, ldc, cos_tab, sin_tab, pos, L, rope_cols};
  return launch_nn<EpiStoreRope, false, false, true>(shape(A, lda, B, ldb, M, N, K), epi, stream);
}

int rv_gemm_nn_swiglu_bf16(const void* A, long lda, const void* B, long ldb, void* GU, long ldgu, void* ACT, long ldact,
                           int M, int N, int K, void* stream) {
  const char* const who = __func__;
  if (M == 0 || N == 0) return 0;
  REQ(K > 0 && K % G2_BK == 0, "K must be a positive multiple of 32");
  REQ(N % 16 == 0, "N (= 2 x ffn, interleaved gate/up columns) must be a multiple of 16");
  CHECK(check_ld(who, {lda, ldb, ldgu}, {ldact}));
  CHECK(check_align(who, {A, B, GU}, 16, "A/B/GU"));
  CHECK(check_align(who, {ACT}, 8, "ACT"));
  return launch_nn(shape(A, lda, B, ldb, M, N, K), EpiSwiGLU{(bf16_t*)GU, ldgu, (bf16_t*)ACT, ldact}, stream);
}

int rv_gemm_nn_swiglu_bwd_bf16(const void* A, long lda, const void* B, long ldb, const void* GU, long ldgu, void* DGU,
                               long lddgu, int M, int N, int K, void* stream) {
  const char* const who = __func__;
  if (M == 0 || N == 0) return 0;
  REQ(K > 0 && K % G2_BK == 0, "K must be a positive multiple of 32");
  REQ(N % 8 == 0, "N (= ffn) must be a multiple of 8");
  CHECK(check_ld(who, {lda, ldb, ldgu, lddgu}, {}));
  CHECK(check_align(who, {A, B, GU, DGU}, 16, "A/B/GU/DGU"));
  return launch_nn(shape(A, lda, B, ldb, M, N, K), EpiSwiGLUBwd{(const bf16_t*)GU, ldgu, (bf16_t*)DGU, lddgu}, stream);
}

int rv_gemm_nn_lora_bf16(const void* A, long lda, const void* B, long ldb, const void* A2, long lda2, const void* B2,
                         long ldb2, int K2, int group_cols, int group0, void* C, long ldc, int M, int N, int K,
                         const void* residual, long ldr, void* stream) {
  const char* const who = __func__;
  if (M == 0 || N == 0) return 0;
  REQ(K > 0 && K % G2_BK == 0 && K2 > 0 && K2 % G2_BK == 0, "K and K2 must be positive multiples of 32");
  REQ(N % 8 == 0 && N >= 8, "N must be a multiple of 8");
  CHECK(check_ld(who, {lda, ldb, lda2, ldb2}, {ldc, residual ? ldr : 0}));
  CHECK(check_align(who, {A, B, A2, B2}, 16, "A/B/A2/B2"));
  CHECK(check_groups(who, group_cols, group0, N, G2_BN));
  const GemmShape g = shape_ext(A, lda, B, ldb, M, N, K, A2, lda2, B2, ldb2, K2, group_cols, group0);
  return launch_nn<EpiStore, true>(g, epi_store(C, ldc, nullptr, residual, ldr, RV_ACT_NONE, 1.0f), stream);
}

// what the fused-adapter entries of the 64-deep-A kernel ask of K and K2
static int check_a64_k(const char* who, int K, int K2) {
  REQ(K >= 512 && K % 64 == 0 && K2 > 0 && K2 % 64 == 0, "K must be a multiple of 64 and >= 512, K2 a positive multiple of 64");
  return 0;
}

// gate|up projection of an ADAPTER model with SwiGLU in the epilogue (round 6): the fused-LoRA K loop
// y = [x | t] [W | B2]^T of rv_gemm_nn_lora_bf16 with the epilogue of rv_gemm_nn_swiglu_bf16.  Interleaved gate / up columns; B2 is the
// EXPANDED adapter matrix [K2 = 2 r][N]: row k < r carries lora_B(gate) on the even columns and zeros on the odd ones, row r + k
// lora_B(up) on the odd columns - peft's adapters are per module, the zeros keep t_gate out of the up columns and vice versa.
int rv_gemm_nn_lora_swiglu_bf16(const void* A, long lda, const void* B, long ldb, const void* A2, long lda2, const void* B2,
                                long ldb2, int K2, void* GU, long ldgu, void* ACT, long ldact, void* ACTD, float p, int seed,
                                int M, int N, int K, void* stream) {
  const char* const who = __func__;
  if (M == 0 || N == 0) return 0;
  CHECK(check_a64_k(who, K, K2));
  REQ(N % 16 == 0, "N (= 2 x ffn, interleaved gate/up columns) must be a multiple of 16");
  CHECK(check_ld(who, {lda, ldb, lda2, ldb2, ldgu}, {ldact}));
  CHECK(check_align(who, {A, B, A2, B2, GU}, 16, "A/B/A2/B2/GU"));
  CHECK(check_align(who, {ACT, ACTD}, 8, "ACT/ACTD"));
  CHECK(check_p(who, p));
  REQ(ACTD == nullptr || ldact == N / 2, "ACTD needs a contiguous ACT");
  EpiSwiGLU epi{(bf16_t*)GU, ldgu, (bf16_t*)ACT, ldact};
  if (ACTD != nullptr && p > 0.f) {
    const DropParams d = drop_params(p, seed);
    epi.ACTD = (bf16_t*)ACTD;
    epi.drop_thresh16 = d.thresh16;
    epi.drop_key = d.key;
    epi.drop_inv_keep = d.inv_keep;
  }
  const GemmShape g = shape_ext(A, lda, B, ldb, M, N, K, A2, lda2, B2, ldb2, K2, 0, 0);
  return launch_nn<EpiSwiGLU, true, false, true>(g, epi, stream);
}

// Input gradient of an ADAPTER model's down projection with the SwiGLU backward in the epilogue: acc = d act = dy W + [mask](dt A) / (1 - p)
// (p > 0: the adapter-first form of rv_gemm_nn_lora_pre_bf16, mask of rv_dropout for the [M][N] activation; p = 0: the in-ring form
// of rv_gemm_nn_lora_bf16), then d(gate|up) from the kept interleaved gate|up tile as rv_gemm_nn_swiglu_bwd_bf16 does.
int rv_gemm_nn_lora_swiglu_bwd_bf16(const void* A, long lda, const void* B, long ldb, const void* A2, long lda2, const void* B2,
                                    long ldb2, int K2, float p, int seed, const void* GU, long ldgu, void* DGU, long lddgu,
                                    int M, int N, int K, void* stream) {
  const char* const who = __func__;
  if (M == 0 || N == 0) return 0;
  CHECK(check_a64_k(who, K, K2));
  REQ(N % 8 == 0, "N (= ffn) must be a multiple of 8");
  CHECK(check_p(who, p));
  CHECK(check_ld(who, {lda, ldb, lda2, ldb2, ldgu, lddgu}, {}));
  CHECK(check_align(who, {A, B, A2, B2, GU, DGU}, 16, "A/B/A2/B2/GU/DGU"));
  GemmShape g = shape_ext(A, lda, B, ldb, M, N, K, A2, lda2, B2, ldb2, K2, 0, 0);
  const EpiSwiGLUBwd epi{(const bf16_t*)GU, ldgu, (bf16_t*)DGU, lddgu};
  if (p == 0.f) return launch_nn<EpiSwiGLUBwd, true, false, true>(g, epi, stream);
  const DropParams d = drop_params(p, seed);
  g.pre_thresh16 = d.thresh16;
  g.pre_key = d.key;
  g.pre_inv_keep = d.inv_keep;
  return launch_nn<EpiSwiGLUBwd, false, true>(g, epi, stream);
}

int rv_gemm_nn_lora_pre_bf16(const void* A, long lda, const void* B, long ldb, const void* A2, long lda2, const void* B2,
                             long ldb2, int K2, int group_cols, int group0, float p, int seed, void* C, long ldc, int M, int N,
                             int K, const void* residual, long ldr, void* stream) {
  const char* const who = __func__;
  if (M == 0 || N == 0) return 0;
  CHECK(check_a64_k(who, K, K2));
  REQ(N % 8 == 0 && N >= 8, "N must be a multiple of 8 (mask layout of rv_dropout)");
  CHECK(check_p(who, p));
  CHECK(check_ld(who, {lda, ldb, lda2, ldb2}, {ldc, residual ? ldr : 0}));
  CHECK(check_align(who, {A, B, A2, B2}, 16, "A/B/A2/B2"));
  CHECK(check_groups(who, group_cols, group0, N, G2_BN));
  GemmShape g = shape_ext(A, lda, B, ldb, M, N, K, A2, lda2, B2, ldb2, K2, group_cols, group0);
  const DropParams d = drop_params(p, seed);
  g.pre_thresh16 = d.thresh16;
  g.pre_key = d.key;
  g.pre_inv_keep = d.inv_keep;
  return launch_nn<EpiStore, false, true>(g, epi_store(C, ldc, nullptr, residual, ldr, RV_ACT_NONE, 1.0f), stream);
}

int rv_gemm_nt_dropout_bf16(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K,
                            const void* residual, long ldr, float alpha, float p, int seed, void* stream) {
  const char* const who = __func__;
  if (M == 0 || N == 0) return 0;
  const GemmShape g = shape(A, lda, B, ldb, M, N, K);
  CHECK(check_shape(g, who));
  CHECK(check_p(who, p));
  REQ(N % 8 == 0, "N must be a multiple of 8 (mask layout of rv_dropout)");
  CHECK(check_ld(who, {}, {ldc, residual ? ldr : 0}));
  EpiStore epi = epi_store(C, ldc, nullptr, residual, ldr, RV_ACT_NONE, alpha);
  const DropParams d = drop_params(p, seed);
  epi.drop_thresh16 = d.thresh16;
  epi.drop_key = d.key;
  epi.drop_inv_keep = d.inv_keep;
  return dispatch(who, g, epi, -1, stream);
}

int rv_gemm_tn_bf16_splitk(const void* P, long ldp, const void* Q, long ldq, void* C, long ldc, int R, int I, int J,
                           float alpha, int splits, float* workspace, void* stream) {
  const char* const who = __func__;
  if (I == 0 || J == 0) return 0;
  REQ(R > 0 && splits >= 1 && splits <= 1024, "R > 0, 1 <= splits <= 1024");
  REQ(I % 8 == 0 && J % 8 == 0, "I and J must be multiples of 8");
  CHECK(check_ld(who, {ldp, ldq}, {ldc}));
  CHECK(check_align(who, {P, Q, workspace}, 16, "P/Q/workspace"));
  REQ(workspace != nullptr, "workspace of splits*I*J floats required");
  const SplitK s = splitk_chunks(R, splits);
  if (launch_gemm_tn((const bf16_t*)P, ldp, (const bf16_t*)Q, ldq, R, I, J, EpiStoreF32{workspace, (long)J}, stream, s.splits,
                     s.r_chunk, (long)I * J))
    return 1;
  return launch_splitk_reduce(workspace, s.splits, I, J, alpha, C, ldc, stream);
}

int rv_gemm_nt_lora_masks_bf16(const void* X, long ldx, const void* A, long lda, void* T, long ldt, int M, int K, int G,
                               float alpha, float p, int seed0, int seed1, int seed2, void* stream) {
  const char* const who = __func__;
  REQ(G >= 1 && G <= 3, "1 <= G <= 3 modules");
  REQ(K > 0 && K % 64 == 0, "K must be a positive multiple of 64");
  CHECK(check_p(who, p));
  CHECK(check_ld(who, {ldx, lda}, {ldt}));
  REQ(M >= 0, "M must not be negative");
  REQ(ldx >= K && lda >= K && ldt >= G * 64, "bad leading dimension (ldx, lda >= K; ldt >= 64 G)");
  if (M == 0) return 0;
  REQ(X && A && T, "X, A and T required");
  CHECK(check_align(who, {X, A}, 16, "X/A"));
  CHECK(check_align(who, {T}, 8, "T"));
  const LoraMasks dm = lora_masks(p, seed0, seed1, seed2);
  return for_modules(G, [&](auto Gc) {
    constexpr int G_ = decltype(Gc)::value, NST = G_ == 1 ? 3 : 2, LDS = NST * (16384 + G_ * 8192);
    const dim3 grid((M + 127) / 128), block(256);
    const bf16_t *x = (const bf16_t*)X, *a = (const bf16_t*)A;
    if (dm.thresh16) return launch<lora_masks_fwd_kernel<G_, NST, true>>(LDS, grid, block, stream, x, ldx, a, lda, (bf16_t*)T, ldt, M, K, alpha, dm);
    return launch<lora_masks_fwd_kernel<G_, NST, false>>(LDS, grid, block, stream, x, ldx, a, lda, (bf16_t*)T, ldt, M, K, alpha, dm);
  });
}

int rv_gemm_nt_dropout_masks_bf16(const void* dT, long lddt, const void* AT, long ldat, void* C, long ldc, int M, int N, int G,
                                  const void* residual, long ldr, float p, int seed0, int seed1, int seed2, void* stream) {
  const char* const who = __func__;
  REQ(G >= 1 && G <= 3, "1 <= G <= 3 modules");
  REQ(N > 0 && N % 64 == 0, "N must be a positive multiple of 64");
  CHECK(check_p(who, p));
  CHECK(check_ld(who, {lddt, ldat}, {ldc, residual ? ldr : 0}));
  REQ(M >= 0, "M must not be negative");
  REQ(lddt >= G * 64 && ldat >= G * 64 && ldc >= N && (residual == nullptr || ldr >= N),
      "bad leading dimension (lddt, ldat >= 64 G; ldc, ldr >= N)");
  if (M == 0) return 0;
  REQ(dT && AT && C, "dT, AT and C required");
  CHECK(check_align(who, {dT, AT}, 16, "dT/AT"));
  CHECK(check_align(who, {C, residual}, 8, "C/residual"));
  // one module: exactly rv_gemm_nt_dropout_bf16 (same kernels, same bits)
  if (G == 1) return rv_gemm_nt_dropout_bf16(dT, lddt, AT, ldat, C, ldc, M, N, 64, residual, ldr, 1.0f, p, seed0, stream);
  const LoraMasks dm = lora_masks(p, seed0, seed1, seed2);
  return for_modules<2>(G, [&](auto Gc) {
    constexpr int G_ = decltype(Gc)::value;
    const dim3 grid(tiles(M, GEMM_BM) * tiles(N, GEMM_BN)), block(GEMM_THREADS);
    const bf16_t *dt = (const bf16_t*)dT, *at = (const bf16_t*)AT, *r = (const bf16_t*)residual;
    if (dm.thresh16) return launch<lora_masks_dgrad_kernel<G_, true>>(GEMM_LDS_BYTES, grid, block, stream, dt, lddt, at, ldat, (bf16_t*)C, ldc, r, ldr, M, N, dm);
    return launch<lora_masks_dgrad_kernel<G_, false>>(GEMM_LDS_BYTES, grid, block, stream, dt, lddt, at, ldat, (bf16_t*)C, ldc, r, ldr, M, N, dm);
  });
}

int rv_gemm_tn_lora_masks_bf16(const void* dT, long lddt, const void* X, long ldx, void* dA, long ldda, int R, int K, int G, float p,
                               int seed0, int seed1, int seed2, int splits, float* workspace, void* stream) {
  const char* const who = __func__;
  REQ(G >= 1 && G <= 3, "1 <= G <= 3 modules");
  REQ(K > 0 && K % 64 == 0, "K must be a positive multiple of 64");
  CHECK(check_p(who, p));
  REQ(R > 0 && splits >= 1 && splits <= 1024, "R > 0, 1 <= splits <= 1024");
  CHECK(check_ld(who, {lddt, ldx}, {ldda}));
  REQ(lddt >= G * 64 && ldx >= K && ldda >= K, "bad leading dimension (lddt >= 64 G; ldx, ldda >= K)");
  REQ(dT && X && dA, "dT, X and dA required");
  CHECK(check_align(who, {dT, X, workspace}, 16, "dT/X/workspace"));
  CHECK(check_align(who, {dA}, 8, "dA"));
  REQ(workspace != nullptr, "workspace of splits * 64 G * K floats required");
  // p = 0: the plain split-K weight gradient
  if (p == 0.f) return rv_gemm_tn_bf16_splitk(dT, lddt, X, ldx, dA, ldda, R, G * 64, K, 1.0f, splits, workspace, stream);
  const SplitK s = splitk_chunks(R, splits);
  const LoraMasks dm = lora_masks(p, seed0, seed1, seed2);
  const int rc = for_modules(G, [&](auto Gc) {
    return launch<lora_masks_wgrad_kernel<decltype(Gc)::value>>(0, dim3(tiles(K, LMW_JT), s.splits), dim3(256), stream,
                                                               (const bf16_t*)dT, lddt, (const bf16_t*)X, ldx, workspace, R, K, s.r_chunk, dm);
  });
  if (rc) return rc;
  return launch_splitk_reduce(workspace, s.splits, G * 64, K, 1.0f, dA, ldda, stream);
}

int rv_gemm_nt_bf16_f32out(const void* A, long lda, const void* B, long ldb, float* C, long ldc, int M, int N, int K,
                           int variant, void* stream) {
  const char* const who = __func__;
  if (M == 0 || N == 0) return 0;
  const GemmShape g = shape(A, lda, B, ldb, M, N, K);
  CHECK(check_shape(g, who));
  CHECK(check_ld(who, {}, {ldc}));
  return dispatch(who, g, EpiStoreF32{C, ldc}, variant, stream);
}

int rv_gemm_nt_bf16_f32res(const void* A, long lda, const void* B, long ldb, float* C, long ldc, int M, int N, int K,
                           const void* bias, const float* residual, long ldr, int variant, void* stream) {
  const char* const who = __func__;
  if (M == 0 || N == 0) return 0;
  const GemmShape g = shape(A, lda, B, ldb, M, N, K);
  CHECK(check_shape(g, who));
  CHECK(check_ld(who, {}, {ldc, ldr}));
  return dispatch(who, g, EpiStoreF32{C, ldc, (const bf16_t*)bias, residual, ldr}, variant, stream);
}

// the vocabulary bounds of the LM-head kernels
static int check_vocab(const char* who, int V, int V_valid) {
  REQ(V_valid > V - 64 && V_valid <= V, "V - 64 < V_valid <= V");
  return 0;
}

int rv_lmhead_logp_fwd(const void* h, long ldh, const void* W, long ldw, const int* tgt, int M, int V, int V_valid, int K,
                       float* pmax, float* psum, float* tgt_logit, int variant, void* stream) {
  const char* const who = __func__;
  if (M == 0) return 0;
  const GemmShape g = shape(h, ldh, W, ldw, M, V, K);
  CHECK(check_shape(g, who));
  REQ(V % 64 == 0, "V, the STORED vocabulary (rows of W), must be a multiple of 64; pad with zero rows");
  CHECK(check_vocab(who, V, V_valid));
  return dispatch(who, g, EpiLogpFwd{tgt, pmax, psum, tgt_logit, V_valid}, variant, stream);
}

int rv_lmhead_logp_bwd(const void* h, long ldh, const void* W, long ldw, const int* tgt, const float* lse,
                       const float* coef, void* dlogits, long ldd, int M, int V, int V_valid, int K, int variant,
                       void* stream) {
  const char* const who = __func__;
  if (M == 0) return 0;
  const GemmShape g = shape(h, ldh, W, ldw, M, V, K);
  CHECK(check_shape(g, who));
  CHECK(check_ld(who, {}, {ldd}));
  CHECK(check_vocab(who, V, V_valid));
  return dispatch(who, g, EpiLogpBwd{tgt, lse, coef, (bf16_t*)dlogits, ldd, V_valid}, variant, stream);
}

}  // extern "C"
