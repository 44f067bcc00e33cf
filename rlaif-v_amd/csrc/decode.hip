// KV-cached candidate generation (the sampling branch of the AI-feedback stage): the three kernels a decode step adds to the
// existing element-wise ops - a weight-streaming skinny NT GEMM (M <= 64 rows), single-query attention against a cache, and the
// temperature / top-p sampler.  Contracts: include/rlaifv_hip.h.
#include <math.h>

#include "common.hpp"
#include "host.hpp"
#include "rlaifv_hip.h"

// ------------------------------------------------------------------ skinny NT GEMM
// One workgroup owns SK_BN = 16 output columns and all M rows: W rows are the MFMA A operand, the activation rows the B
// operand (C^T tiles), both fetched from global memory straight into fragments.  Inside a 64-deep K chunk lane group g =
// lane >> 4 takes k = 16 g .. 16 g + 15 (32 contiguous bytes per lane, a full 128-byte line per W row and wave) and feeds
// elements 0..7 to the first MFMA and 8..15 to the second; both operands use the same map, so the sum over k is complete.
// The 8 waves take the chunks round-robin and their partial tiles are added in wave order through LDS: every output
// element is a function of its own A row and W row only - the same bits at any M.
#define SK_BN 16
#define SK_WAVES 8
#define SK_DEPTH 4      // chunks per trip of the deep loop

template <int MT, bool F32OUT>
__global__ __launch_bounds__(SK_WAVES * 64) void gemm_nt_skinny_kernel(const bf16_t* __restrict__ A, long lda,
                                                                         const bf16_t* __restrict__ W, long ldw,
                                                                         void* __restrict__ C, long ldc,
                                                                         const bf16_t* __restrict__ R, long ldr, int M, int N,
                                                                         int K) {
  __shared__ f32x4_t part[SK_WAVES][MT][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * SK_BN, r16 = lane & 15, g = lane >> 4;
  const int wrow = min(n0 + r16, N - 1);                       // edge panel: re-read the last row, never a row past N
  const bf16_t* wp = W + (long)wrow * ldw + 16 * g;
  const bf16_t* xp[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) xp[t] = A + (long)min(t * 16 + r16, M - 1) * lda + 16 * g;
  f32x4_t acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int nch = K >> 6;
  // A wave's chunks are wave, wave + 8, ...: the deep loop takes SK_DEPTH of them per trip and names all their loads ahead of
  // their MFMAs, then single chunks follow; the accumulation order is the chunk order either way.  What hipcc makes of the deep
  // loop (gfx950, -O3) is NOT four chunks in flight: it spreads the loads between the MFMAs - at MT = 4 eight 16-byte loads
  // before the first wait, then one or two per MFMA at vmcnt 5..7 and vmcnt(0) at the end of a trip, i.e. under one chunk (10
  // loads) ahead; at MT = 1 eight of a trip's 16.  A wave therefore has 5 - 8 loads (80 - 128 bytes per lane) outstanding, and
  // the weight stream's latency is covered by the waves resident on a CU (at most 94 VGPRs: two workgroups, 16 waves).
  int c = wave;
  for (; c + (SK_DEPTH - 1) * SK_WAVES < nch; c += SK_DEPTH * SK_WAVES) {
    bf16x8_t w0[SK_DEPTH], w1[SK_DEPTH], x0[SK_DEPTH][MT], x1[SK_DEPTH][MT];
#pragma unroll
    for (int u = 0; u < SK_DEPTH; ++u) {
      const long k0 = (long)(c + u * SK_WAVES) << 6;
      w0[u] = *(const bf16x8_t*)(wp + k0);
      w1[u] = *(const bf16x8_t*)(wp + k0 + 8);
    }
#pragma unroll
    for (int u = 0; u < SK_DEPTH; ++u) {
      const long k0 = (long)(c + u * SK_WAVES) << 6;
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        x0[u][t] = *(const bf16x8_t*)(xp[t] + k0);
        x1[u][t] = *(const bf16x8_t*)(xp[t] + k0 + 8);
      }
    }
#pragma unroll
    for (int u = 0; u < SK_DEPTH; ++u) {
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0[u], x0[u][t], acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1[u], x1[u][t], acc[t], 0, 0, 0);
      }
    }
  }
  for (; c < nch; c += SK_WAVES) {
    const long k0 = (long)c << 6;
    const bf16x8_t w0 = *(const bf16x8_t*)(wp + k0), w1 = *(const bf16x8_t*)(wp + k0 + 8);
    bf16x8_t x0[MT], x1[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      x0[t] = *(const bf16x8_t*)(xp[t] + k0);
      x1[t] = *(const bf16x8_t*)(xp[t] + k0 + 8);
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, x0[t], acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, x1[t], acc[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < MT; ++t) part[wave][t][lane] = acc[t];
  __syncthreads();
  if (tid < MT * 64) {
    const int t = tid >> 6;
    f32x4_t s = part[0][t][lane];
#pragma unroll
    for (int w = 1; w < SK_WAVES; ++w) s += part[w][t][lane];
    const int m = t * 16 + r16, n = n0 + 4 * g;               // accumulator: column = lane & 15 (m), rows 4 g .. 4 g + 3 (n)
    if (m < M && n < N) {                                      // N % 4 == 0: the four columns are inside together
      if (R) {
        const uint2 rr = *(const uint2*)(R + (long)m * ldr + n);
        s[0] += bf2f((bf16_t)(rr.x & 0xffffu));
        s[1] += bf2f((bf16_t)(rr.x >> 16));
        s[2] += bf2f((bf16_t)(rr.y & 0xffffu));
        s[3] += bf2f((bf16_t)(rr.y >> 16));
      }
      if constexpr (F32OUT) {
        *(f32x4_t*)((float*)C + (long)m * ldc + n) = s;
      } else {
        uint2 o;
        o.x = pack2bf(s[0], s[1]);
        o.y = pack2bf(s[2], s[3]);
        *(uint2*)((bf16_t*)C + (long)m * ldc + n) = o;
      }
    }
  }
}

template <int MT>
static int launch_skinny(const void* A, long lda, const void* W, long ldw, void* C, long ldc, const void* R, long ldr, int M,
                          int N, int K, int out_f32, void* stream) {
  const dim3 grid((N + SK_BN - 1) / SK_BN), block(SK_WAVES * 64);
  if (out_f32)
    return launch<gemm_nt_skinny_kernel<MT, true>>(0, grid, block, stream, (const bf16_t*)A, lda, (const bf16_t*)W, ldw, C, ldc,
                                                   (const bf16_t*)R, ldr, M, N, K);
  return launch<gemm_nt_skinny_kernel<MT, false>>(0, grid, block, stream, (const bf16_t*)A, lda, (const bf16_t*)W, ldw, C, ldc,
                                                  (const bf16_t*)R, ldr, M, N, K);
}

extern "C" int rv_gemm_nt_skinny_bf16(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K,
                                      const void* residual, long ldr, int out_f32, void* stream) {
  RV_REQUIRE(M >= 1 && M <= 64, "rv_gemm_nt_skinny_bf16: 1 <= M <= 64");
  RV_REQUIRE(K > 0 && K % 64 == 0, "rv_gemm_nt_skinny_bf16: K must be a positive multiple of 64");
  RV_REQUIRE(N > 0 && N % 4 == 0, "rv_gemm_nt_skinny_bf16: N must be a positive multiple of 4");
  RV_REQUIRE(A && W && C, "rv_gemm_nt_skinny_bf16: NULL operand");
  RV_REQUIRE(out_f32 == 0 || out_f32 == 1, "rv_gemm_nt_skinny_bf16: out_f32 is 0 (bf16 C) or 1 (fp32 C)");
  RV_REQUIRE(lda % 8 == 0 && ldw % 8 == 0 && lda >= K && ldw >= K, "rv_gemm_nt_skinny_bf16: lda / ldw: multiples of 8, >= K");
  RV_REQUIRE(ldc % 4 == 0 && ldc >= N, "rv_gemm_nt_skinny_bf16: ldc: a multiple of 4, >= N");
  RV_REQUIRE((((uintptr_t)A | (uintptr_t)W) & 15) == 0, "rv_gemm_nt_skinny_bf16: A / W must be 16-byte aligned");
  RV_REQUIRE(((uintptr_t)C & (out_f32 ? 15 : 7)) == 0, "rv_gemm_nt_skinny_bf16: C alignment (8 bytes bf16, 16 bytes fp32)");
  RV_REQUIRE(residual == nullptr || (ldr % 4 == 0 && ldr >= N && ((uintptr_t)residual & 7) == 0),
             "rv_gemm_nt_skinny_bf16: residual: ldr a multiple of 4, >= N, 8-byte aligned");
  switch ((M + 15) / 16) {
    case 1: return launch_skinny<1>(A, lda, W, ldw, C, ldc, residual, ldr, M, N, K, out_f32, stream);
    case 2: return launch_skinny<2>(A, lda, W, ldw, C, ldc, residual, ldr, M, N, K, out_f32, stream);
    case 3: return launch_skinny<3>(A, lda, W, ldw, C, ldc, residual, ldr, M, N, K, out_f32, stream);
    default: return launch_skinny<4>(A, lda, W, ldw, C, ldc, residual, ldr, M, N, K, out_f32, stream);
  }
}

// ------------------------------------------------------------------ decode attention
// One workgroup per (sequence, kv head, key split), 4 waves.  A 16-lane group reads one 256-byte K (then V) row, 16 bytes
// per lane straight into registers, and serves the G query heads of the kv head with it; the 16 groups of the workgroup
// take the split's keys round-robin, four keys per group in flight, each with its own online softmax (fp32, base 2).  The
// groups are merged inside a wave by two butterfly steps and across the waves in wave order through LDS: fixed order.
#define AD_HD 128
#define AD_WS 132        // floats per (sequence, head, split) of the workspace: m, l, 2 unused, o[128]

__device__ __forceinline__ void ad_unpack8(const uint4 v, float* f) {
  f[0] = __uint_as_float(v.x << 16), f[1] = __uint_as_float(v.x & 0xffff0000u);
  f[2] = __uint_as_float(v.y << 16), f[3] = __uint_as_float(v.y & 0xffff0000u);
  f[4] = __uint_as_float(v.z << 16), f[5] = __uint_as_float(v.z & 0xffff0000u);
  f[6] = __uint_as_float(v.w << 16), f[7] = __uint_as_float(v.w & 0xffff0000u);
}
__device__ __forceinline__ float ad_w(float m, float mn) { return m == -INFINITY ? 0.f : exp2f(m - mn); }

// IDX (rv_attn_decode_indexed): the sequence's own span is a row table, `own_off` = own_rows [M][ld_rows]; an entry is clamped
// to the cache's rows [0, kv_rows), so a bad table reads wrong rows and never memory outside the cache.
template <int G, bool IDX>
__global__ __launch_bounds__(256) void attn_decode_kernel(const bf16_t* __restrict__ q, long ldq,
                                                          const bf16_t* __restrict__ kv, long ldkv, int k_col0, int v_col0,
                                                          const int* __restrict__ pre_off, const int* __restrict__ pre_len,
                                                          const int* __restrict__ own_off, const int* __restrict__ own_len,
                                                          int H, int n_split, float scale_log2e, float* __restrict__ ws,
                                                          long ld_rows, int kv_rows) {
  __shared__ float sm[4][G][AD_HD + 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, dsub = lane & 15, ksub = lane >> 4;
  const int g = blockIdx.x / n_split, sp = blockIdx.x % n_split, m = blockIdx.y;
  const int pl = pre_len[m], po = pre_off[m], oo = IDX ? 0 : own_off[m];
  const int T = pl + (IDX ? min(own_len[m], (int)ld_rows) : own_len[m]);      // IDX: never past the table's row
  const int* tab = own_off + (long)m * ld_rows;              // IDX only
  const int chunk = (T + n_split - 1) / n_split;
  const int t0 = sp * chunk, t1 = min(T, t0 + chunk);
  float qf[G][8], o[G][8], mx[G], l[G];
#pragma unroll
  for (int j = 0; j < G; ++j) {
    ad_unpack8(*(const uint4*)(q + (long)m * ldq + (long)(g * G + j) * AD_HD + 8 * dsub), qf[j]);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[j][e] = 0.f;
    mx[j] = -INFINITY, l[j] = 0.f;
  }
  const long kc = (long)k_col0 + (long)g * AD_HD + 8 * dsub, vc = (long)v_col0 + (long)g * AD_HD + 8 * dsub;
  for (int t = t0 + wave * 4 + ksub; t < t1; t += 64) {
    uint4 kr[4], vr[4];
    if constexpr (IDX) {
      long row[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {                           // the batch's table entries first: four loads in flight, then K / V
        const int tt = min(t + 16 * b, t1 - 1);
        row[b] = tt < pl ? (long)po + tt : (long)min(max(tab[tt - pl], 0), kv_rows - 1);
      }
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        kr[b] = *(const uint4*)(kv + row[b] * ldkv + kc);
        vr[b] = *(const uint4*)(kv + row[b] * ldkv + vc);
      }
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int tt = min(t + 16 * b, t1 - 1);               // a key past the split: re-read its last row, weight 0 below
        const long row = tt < pl ? (long)po + tt : (long)oo + (tt - pl);
        kr[b] = *(const uint4*)(kv + row * ldkv + kc);
        vr[b] = *(const uint4*)(kv + row * ldkv + vc);
      }
    }
    float s[4][G];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      float kf[8];
      ad_unpack8(kr[b], kf);
#pragma unroll
      for (int j = 0; j < G; ++j) {
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) d += qf[j][e] * kf[e];
        d += __shfl_xor(d, 1, 64);
        d += __shfl_xor(d, 2, 64);
        d += __shfl_xor(d, 4, 64);
        d += __shfl_xor(d, 8, 64);
        s[b][j] = (t + 16 * b < t1) ? d * scale_log2e : -INFINITY;     // base-2 score: (q . k) * fl(scale * log2 e)
      }
    }
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const float mn = fmaxf(fmaxf(mx[j], fmaxf(s[0][j], s[1][j])), fmaxf(s[2][j], s[3][j]));   // finite: key t is valid
      const float a = exp2f(mx[j] - mn);                       // exp2(-inf) = 0 on the first batch
      l[j] *= a;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[j][e] *= a;
      mx[j] = mn;
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      float vf[8];
      ad_unpack8(vr[b], vf);
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const float p = exp2f(s[b][j] - mx[j]);
        l[j] += p;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[j][e] += p * vf[e];
      }
    }
  }
  // the wave's four key groups -> one (lanes differing in bits 4 and 5 hold the same dims of different keys)
#pragma unroll
  for (int off = 16; off <= 32; off <<= 1) {
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const float m2 = __shfl_xor(mx[j], off, 64), l2 = __shfl_xor(l[j], off, 64);
      const float mn = fmaxf(mx[j], m2), a = ad_w(mx[j], mn), b = ad_w(m2, mn);
      l[j] = l[j] * a + l2 * b;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[j][e] = o[j][e] * a + __shfl_xor(o[j][e], off, 64) * b;
      mx[j] = mn;
    }
  }
  if (ksub == 0) {
#pragma unroll
    for (int j = 0; j < G; ++j) {
      if (dsub == 0) sm[wave][j][AD_HD] = mx[j], sm[wave][j][AD_HD + 1] = l[j];
#pragma unroll
      for (int e = 0; e < 8; ++e) sm[wave][j][8 * dsub + e] = o[j][e];
    }
  }
  __syncthreads();
  for (int i = tid; i < G * AD_HD; i += 256) {
    const int j = i >> 7, d = i & (AD_HD - 1);
    float mn = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) mn = fmaxf(mn, sm[w][j][AD_HD]);
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float c = ad_w(sm[w][j][AD_HD], mn);
      L += sm[w][j][AD_HD + 1] * c;
      O += sm[w][j][d] * c;
    }
    float* dst = ws + (((long)m * H + (g * G + j)) * n_split + sp) * AD_WS;
    dst[4 + d] = O;
    if (d == 0) dst[0] = mn, dst[1] = L;                       // an empty split: m = -inf, l = 0, o = 0
  }
}

__global__ __launch_bounds__(AD_HD) void attn_decode_combine_kernel(const float* __restrict__ ws, int n_split,
                                                                    bf16_t* __restrict__ out, long ldo,
                                                                    float* __restrict__ lse, int H) {
  const int h = blockIdx.x, m = blockIdx.y, d = threadIdx.x;
  const float* src = ws + ((long)m * H + h) * n_split * AD_WS;
  float mn = -INFINITY;
  for (int s = 0; s < n_split; ++s) mn = fmaxf(mn, src[(long)s * AD_WS]);
  float L = 0.f, O = 0.f;
  for (int s = 0; s < n_split; ++s) {
    const float c = ad_w(src[(long)s * AD_WS], mn);            // a split without keys: weight 0, never NaN
    L += src[(long)s * AD_WS + 1] * c;
    O += src[(long)s * AD_WS + 4 + d] * c;
  }
  out[(long)m * ldo + (long)h * AD_HD + d] = f2bf(L > 0.f ? O / L : 0.f);
  if (lse && d == 0) lse[(long)m * H + h] = (mn + log2f(L)) * 0.6931471805599453f;
}

extern "C" long rv_attn_decode_workspace_floats(int M, int H, int n_split) {
  if (M < 1 || H < 1 || n_split < 1) return 0;
  return (long)M * H * n_split * AD_WS;
}

// the argument checks and the two launches that rv_attn_decode and rv_attn_decode_indexed share
template <bool IDX>
static int attn_decode_run(const char* who, const void* q, long ldq, const void* kv, long ldkv, int k_col0, int v_col0,
                           const int* pre_off, const int* pre_len, const int* own, long ld_rows, int kv_rows, const int* own_len,
                           void* out, long ldo, float* lse, int M, int H, int hd, int kv_group, float scale, int n_split,
                           float* workspace, long workspace_floats, void* stream) {
  RV_REQUIRE_AS(who, hd == AD_HD, "hd must be 128");
  RV_REQUIRE_AS(who, M >= 1 && M <= 65535 && H >= 1, "1 <= M <= 65535, H >= 1");
  RV_REQUIRE_AS(who, kv_group == 1 || kv_group == 2 || kv_group == 4 || kv_group == 8, "kv_group in {1, 2, 4, 8}");
  RV_REQUIRE_AS(who, H % kv_group == 0, "kv_group must divide H");
  RV_REQUIRE_AS(who, n_split >= 1 && n_split <= 256, "1 <= n_split <= 256");
  RV_REQUIRE_AS(who, q && kv && out && pre_off && pre_len && own && own_len && workspace, "NULL buffer");
  RV_REQUIRE_AS(who, workspace_floats >= rv_attn_decode_workspace_floats(M, H, n_split),
                "workspace smaller than rv_attn_decode_workspace_floats(M, H, n_split)");
  RV_REQUIRE_AS(who, ldq % 8 == 0 && ldkv % 8 == 0 && k_col0 % 8 == 0 && v_col0 % 8 == 0 && k_col0 >= 0 && v_col0 >= 0,
                "ldq, ldkv, k_col0, v_col0 must be multiples of 8");
  RV_REQUIRE_AS(who, ldq >= (long)H * hd && ldo >= (long)H * hd, "ldq / ldo smaller than H * hd");
  RV_REQUIRE_AS(who, (((uintptr_t)q | (uintptr_t)kv | (uintptr_t)workspace) & 15) == 0, "q / kv / workspace 16-byte aligned");
  const int nkv = H / kv_group;
  const dim3 grid(nkv * n_split, M), block(256);
  const float sl2 = scale * 1.4426950408889634f;
#define AD_LAUNCH(G)                                                                                                         \
  launch<attn_decode_kernel<G, IDX>>(0, grid, block, stream, (const bf16_t*)q, ldq, (const bf16_t*)kv, ldkv, k_col0, v_col0, \
                                     pre_off, pre_len, own, own_len, H, n_split, sl2, workspace, ld_rows, kv_rows)
  int rc;
  switch (kv_group) {
    case 1: rc = AD_LAUNCH(1); break;
    case 2: rc = AD_LAUNCH(2); break;
    case 4: rc = AD_LAUNCH(4); break;
    default: rc = AD_LAUNCH(8); break;
  }
#undef AD_LAUNCH
  if (rc) return rc;
  return launch<attn_decode_combine_kernel>(0, dim3(H, M), dim3(AD_HD), stream, workspace, n_split, (bf16_t*)out, ldo, lse, H);
}

extern "C" int rv_attn_decode(const void* q, long ldq, const void* kv, long ldkv, int k_col0, int v_col0, const int* pre_off,
                              const int* pre_len, const int* own_off, const int* own_len, void* out, long ldo, float* lse,
                              int M, int H, int hd, int kv_group, float scale, int n_split, float* workspace,
                              long workspace_floats, void* stream) {
  return attn_decode_run<false>("rv_attn_decode", q, ldq, kv, ldkv, k_col0, v_col0, pre_off, pre_len, own_off, 0, 0, own_len, out,
                                ldo, lse, M, H, hd, kv_group, scale, n_split, workspace, workspace_floats, stream);
}

extern "C" int rv_attn_decode_indexed(const void* q, long ldq, const void* kv, long ldkv, int kv_rows, int k_col0, int v_col0,
                                      const int* pre_off, const int* pre_len, const int* own_rows, long ld_rows, int cur_own_len,
                                      const int* own_len, void* out, long ldo, float* lse, int M, int H, int hd, int kv_group,
                                      float scale, int n_split, float* workspace, long workspace_floats, void* stream) {
  RV_REQUIRE(kv_rows >= 1, "rv_attn_decode_indexed: kv_rows (rows of the cache) must be >= 1");
  RV_REQUIRE(cur_own_len >= 0 && ld_rows >= cur_own_len && ld_rows >= 1,
             "rv_attn_decode_indexed: ld_rows must be >= 1 and >= the current own length");
  RV_REQUIRE(((uintptr_t)own_rows & 3) == 0, "rv_attn_decode_indexed: own_rows must be 4-byte aligned");
  return attn_decode_run<true>("rv_attn_decode_indexed", q, ldq, kv, ldkv, k_col0, v_col0, pre_off, pre_len, own_rows, ld_rows,
                               kv_rows, own_len, out, ldo, lse, M, H, hd, kv_group, scale, n_split, workspace, workspace_floats,
                               stream);
}

// ------------------------------------------------------------------ sampler
// One workgroup of 1024 threads per row; thread t keeps vocabulary ids [t IPT, (t + 1) IPT) in registers, so the index
// order of the inverse-CDF draw is thread order.  Every reduction is a wave butterfly followed by a sum / min / max over the
// 16 wave results in wave order: fixed.
#define ST_THREADS 1024

__device__ __forceinline__ int block_min_i(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = red[0];
  for (int i = 1; i < (int)(blockDim.x >> 6); ++i) r = min(r, red[i]);
  return r;
}

// the number of ids counted over the workgroup: wave butterfly, then the 16 wave counts
__device__ __forceinline__ int block_count(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = 0;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) r += red[i];
  return r;
}

// TOPK (rv_sample_token_topk with 0 < top_k < V while sampling) adds step 2b between the scores and the softmax; TOPK = false is
// rv_sample_token's kernel as it was, top_k unread.
template <int IPT, bool TOPK>
__global__ __launch_bounds__(ST_THREADS) void sample_token_kernel(const float* __restrict__ logits, long ldl, int V,
                                                                  const int* __restrict__ seen_off,
                                                                  const int* __restrict__ seen_ids, float penalty,
                                                                  float temperature, float top_p,
                                                                  const float* __restrict__ u, int vec,
                                                                  int* __restrict__ token, float* __restrict__ logp,
                                                                  int top_k) {
  extern __shared__ uint32_t st_bits[];            // [ceil(V / 32)] when the penalty is on
  __shared__ float red[16];
  __shared__ int redi[16];
  __shared__ float red_mx[16];
  __shared__ int red_ix[16];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* row = logits + (long)m * ldl;
  const bool pen = seen_off != nullptr && penalty != 1.0f;
  if (pen) {
    const int nw = (V + 31) >> 5;
    for (int i = tid; i < nw; i += ST_THREADS) st_bits[i] = 0u;
    __syncthreads();
    for (int i = seen_off[m] + tid; i < seen_off[m + 1]; i += ST_THREADS) {
      const int id = seen_ids[i];
      if (id >= 0 && id < V) atomicOr(&st_bits[id >> 5], 1u << (id & 31));
    }
    __syncthreads();
  }
  const bool greedy = temperature == 0.f;
  const float tdiv = greedy ? 1.f : temperature;
  auto value = [&](int i, float l) {
    if (pen && ((st_bits[i >> 5] >> (i & 31)) & 1u)) l = l > 0.f ? l / penalty : l * penalty;
    return l / tdiv;
  };
  const int base = tid * IPT;
  float p[IPT];
  if (vec && base + IPT <= V) {
#pragma unroll
    for (int e = 0; e < IPT; e += 4) {
      const float4 v4 = *(const float4*)(row + base + e);
      p[e] = v4.x, p[e + 1] = v4.y, p[e + 2] = v4.z, p[e + 3] = v4.w;
    }
  } else {
#pragma unroll
    for (int e = 0; e < IPT; ++e) p[e] = base + e < V ? row[base + e] : -INFINITY;
  }
  float mx = -INFINITY;
  int ix = 0x7fffffff;
#pragma unroll
  for (int e = 0; e < IPT; ++e) {
    if (base + e < V) {
      p[e] = value(base + e, p[e]);
      if (p[e] > mx) mx = p[e], ix = base + e;        // indices grow inside a thread: the first of equal maxima stays
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(mx, o, 64);
    const int i2 = __shfl_xor(ix, o, 64);
    if (m2 > mx || (m2 == mx && i2 < ix)) mx = m2, ix = i2;
  }
  if (lane == 0) red_mx[wave] = mx, red_ix[wave] = ix;
  __syncthreads();
  mx = red_mx[0], ix = red_ix[0];
  for (int w = 1; w < ST_THREADS / 64; ++w)
    if (red_mx[w] > mx || (red_mx[w] == mx && red_ix[w] < ix)) mx = red_mx[w], ix = red_ix[w];
  const float x_top = mx;
  if constexpr (TOPK) {
    // TopKLogitsWarper without the sort: tau = the largest score with at least top_k scores >= it, built bit by bit from the top
    // on score_key (integer order = float order, so distinct scores never merge as their probabilities can); scores below tau
    // leave, everything tied with it stays.  The keys take the scores' registers for the 32 counts; ids behind the row get
    // key 0, below every score's.
#pragma unroll
    for (int e = 0; e < IPT; ++e) p[e] = __uint_as_float(base + e < V ? score_key(p[e]) : 0u);
    uint32_t tk = 0u;
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t c = tk | (1u << bit);
      int n = 0;
#pragma unroll
      for (int e = 0; e < IPT; ++e) n += __float_as_uint(p[e]) >= c ? 1 : 0;
      if (block_count(n, redi) >= top_k) tk = c;
    }
#pragma unroll
    for (int e = 0; e < IPT; ++e) p[e] = __float_as_uint(p[e]) < tk ? -INFINITY : score_of_key(__float_as_uint(p[e]));
  }
  float loc = 0.f;
#pragma unroll
  for (int e = 0; e < IPT; ++e) {
    p[e] = (base + e < V && p[e] != -INFINITY) ? expf(p[e] - x_top) : 0.f;
    loc += p[e];
  }
  const float Z = block_sum(loc, red);
  if (greedy) {
    if (tid == 0) {
      token[m] = ix;
      logp[m] = (value(ix, row[ix]) - x_top) - logf(Z);
    }
    return;
  }
  if (top_p < 1.f) {
    // TopPLogitsWarper without the sort: a token of probability v is dropped iff the mass of all tokens <= v is <= 1 - top_p;
    // that mass grows with v, so bisect the bit pattern of v (non-negative floats order like their bits) for the smallest kept value.
    const float c = (1.f - top_p) * Z;
    uint32_t lo = 0u, hi = __float_as_uint(1.f);      // f(lo) false (mass 0), f(hi) true (the top token has p = exp(0) = 1)
    while (hi - lo > 1u) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      const float v = __uint_as_float(mid);
      float sacc = 0.f;
#pragma unroll
      for (int e = 0; e < IPT; ++e) sacc += p[e] <= v ? p[e] : 0.f;
      if (block_sum(sacc, red) > c) hi = mid; else lo = mid;
    }
    const float tau = __uint_as_float(hi);
    loc = 0.f;
#pragma unroll
    for (int e = 0; e < IPT; ++e) {
      p[e] = p[e] >= tau ? p[e] : 0.f;
      loc += p[e];
    }
  }
  const float Zk = top_p < 1.f ? block_sum(loc, red) : Z;
  // exclusive prefix of the thread totals in thread (= vocabulary) order
  float inc = loc;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float n = __shfl_up(inc, o, 64);
    if (lane >= o) inc += n;
  }
  __syncthreads();
  if (lane == 63) red[wave] = inc;
  __syncthreads();
  float run = inc - loc;
  for (int w = 0; w < wave; ++w) run += red[w];
  const float target = u[m] * Zk;
  int found = 0x7fffffff, last = -1;
#pragma unroll
  for (int e = 0; e < IPT; ++e) {
    if (p[e] > 0.f) {
      run += p[e];
      last = base + e;
      if (run > target && found == 0x7fffffff) found = base + e;
    }
  }
  found = block_min_i(found, redi);
  last = -block_min_i(-last, redi);
  if (tid == 0) {
    const int tok = found != 0x7fffffff ? found : last;       // u Zk rounded past the total: the last kept token
    token[m] = tok;
    logp[m] = (value(tok, row[tok]) - x_top) - logf(Zk);
  }
}

// top_k off (0, >= V_valid) or greedy: rv_sample_token's kernel, whichever entry point asks
static int sample_token_launch(const float* logits, long ldl, int M, int V_valid, const int* seen_off, const int* seen_ids,
                               float penalty, float temperature, float top_p, int top_k, const float* u, int* token, float* logp,
                               void* stream) {
  const bool pen = seen_off != nullptr && penalty != 1.0f;
  const int lds = pen ? (V_valid + 31) / 32 * 4 : 0;
  const int vec = (((uintptr_t)logits & 15) == 0 && ldl % 4 == 0) ? 1 : 0;
  const bool topk = top_k > 0 && top_k < V_valid && temperature != 0.f;
#define ST_LAUNCH(IPT, TOPK)                                                                                                   \
  launch<sample_token_kernel<IPT, TOPK>>(lds, dim3(M), dim3(ST_THREADS), stream, logits, ldl, V_valid, seen_off, seen_ids, penalty, \
                                         temperature, top_p, u, vec, token, logp, top_k)
  if (V_valid <= ST_THREADS * 8) return topk ? ST_LAUNCH(8, true) : ST_LAUNCH(8, false);
  if (V_valid <= ST_THREADS * 32) return topk ? ST_LAUNCH(32, true) : ST_LAUNCH(32, false);
  return topk ? ST_LAUNCH(64, true) : ST_LAUNCH(64, false);
#undef ST_LAUNCH
}

extern "C" int rv_sample_token(const float* logits, long ldl, int M, int V_valid, const int* seen_off, const int* seen_ids,
                               float penalty, float temperature, float top_p, const float* u, int* token, float* logp,
                               void* stream) {
  RV_REQUIRE(M > 0 && V_valid > 0 && ldl >= V_valid, "rv_sample_token: M, V_valid > 0, ldl >= V_valid");
  RV_REQUIRE(V_valid <= ST_THREADS * 64, "rv_sample_token: V_valid <= 65536 (the row is held in registers)");
  RV_REQUIRE(logits && token && logp, "rv_sample_token: NULL buffer");
  RV_REQUIRE(temperature >= 0.f, "rv_sample_token: temperature must be >= 0 (0 = greedy)");
  RV_REQUIRE(top_p > 0.f, "rv_sample_token: top_p must be > 0 (>= 1 keeps every token)");
  RV_REQUIRE(penalty > 0.f, "rv_sample_token: the repetition penalty must be positive (1 = off)");
  RV_REQUIRE(temperature == 0.f || u != nullptr, "rv_sample_token: sampling needs the uniforms u[M]");
  RV_REQUIRE(seen_off == nullptr || seen_ids != nullptr, "rv_sample_token: seen_off without seen_ids");
  return sample_token_launch(logits, ldl, M, V_valid, seen_off, seen_ids, penalty, temperature, top_p, 0, u, token, logp, stream);
}

extern "C" int rv_sample_token_topk(const float* logits, long ldl, int M, int V_valid, const int* seen_off, const int* seen_ids,
                                    float penalty, float temperature, float top_p, int top_k, const float* u, int* token,
                                    float* logp, void* stream) {
  RV_REQUIRE(M > 0 && V_valid > 0 && ldl >= V_valid, "rv_sample_token_topk: M, V_valid > 0, ldl >= V_valid");
  RV_REQUIRE(V_valid <= ST_THREADS * 64, "rv_sample_token_topk: V_valid <= 65536 (the row is held in registers)");
  RV_REQUIRE(logits && token && logp, "rv_sample_token_topk: NULL buffer");
  RV_REQUIRE(temperature >= 0.f, "rv_sample_token_topk: temperature must be >= 0 (0 = greedy)");
  RV_REQUIRE(top_p > 0.f, "rv_sample_token_topk: top_p must be > 0 (>= 1 keeps every token)");
  RV_REQUIRE(top_k >= 0, "rv_sample_token_topk: top_k must be >= 0 (0 or >= V_valid keeps every token)");
  RV_REQUIRE(penalty > 0.f, "rv_sample_token_topk: the repetition penalty must be positive (1 = off)");
  RV_REQUIRE(temperature == 0.f || u != nullptr, "rv_sample_token_topk: sampling needs the uniforms u[M]");
  RV_REQUIRE(seen_off == nullptr || seen_ids != nullptr, "rv_sample_token_topk: seen_off without seen_ids");
  return sample_token_launch(logits, ldl, M, V_valid, seen_off, seen_ids, penalty, temperature, top_p, top_k, u, token, logp, stream);
}
