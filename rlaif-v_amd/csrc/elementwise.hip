// HBM-bound kernels of the DPO step (norms, RoPE, SwiGLU, GELU, transposes, splice, optimizer).
// All bf16 traffic is 16 bytes per lane (8 x bf16); accumulation in fp32.
#include "common.hpp"
#include "host.hpp"
#include "rlaifv_hip.h"

namespace {

__device__ __forceinline__ void unpack8(const uint4& v, float (&f)[8]) {
  f[0] = bf2f((bf16_t)(v.x & 0xffff)); f[1] = bf2f((bf16_t)(v.x >> 16));
  f[2] = bf2f((bf16_t)(v.y & 0xffff)); f[3] = bf2f((bf16_t)(v.y >> 16));
  f[4] = bf2f((bf16_t)(v.z & 0xffff)); f[5] = bf2f((bf16_t)(v.z >> 16));
  f[6] = bf2f((bf16_t)(v.w & 0xffff)); f[7] = bf2f((bf16_t)(v.w >> 16));
}
__device__ __forceinline__ uint4 pack8(const float (&f)[8]) {
  uint4 v;
  v.x = pack2bf(f[0], f[1]); v.y = pack2bf(f[2], f[3]);
  v.z = pack2bf(f[4], f[5]); v.w = pack2bf(f[6], f[7]);
  return v;
}

// rv_dropout applied to one 16-byte chunk (8 bf16 values, chunk index i8 in the CONTIGUOUS tensor the mask is defined on): the
// arithmetic of dropout_kernel, so a producer kernel can emit the dropped copy of its output bit-identically
__device__ __forceinline__ uint4 dropout_chunk(const uint4 v, long i8, uint32_t thresh16, float inv_keep, uint32_t key) {
  float f[8];
  unpack8(v, f);
  const uint32_t base = drop_base((uint32_t)(i8 >> 30), key);
#pragma unroll
  for (int j = 0; j < 4; ++j) drop_keep2(drop_pair_bits((uint32_t)i8 * 4u + (uint32_t)j, base), thresh16, inv_keep, f[2 * j], f[2 * j + 1]);
  return pack8(f);
}

// 8 consecutive elements of a bf16 or an fp32 row as floats (the fp32 forms carry the opt-in fp32 residual streams)
__device__ __forceinline__ void ln_load8(const bf16_t* p, float (&f)[8]) { unpack8(*(const uint4*)p, f); }
__device__ __forceinline__ void ln_load8(const float* p, float (&f)[8]) {
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

// ------------------------------------------------------------------ RMSNorm
// DROP: also writes yd = rv_dropout(y) (contiguous [rows][d], mask index r * d + c): the LoRA branch input of the projection that
// follows, without a second pass over y
template <bool DROP>
__global__ __launch_bounds__(256) void rmsnorm_fwd_kernel(const bf16_t* __restrict__ x, long ldx,
                                                          const int* __restrict__ row_idx,
                                                          const bf16_t* __restrict__ w, bf16_t* __restrict__ y,
                                                          long ldy, float* __restrict__ rstd_out, int rows, int d,
                                                          float eps, bf16_t* __restrict__ yd, uint32_t thresh16,
                                                          float inv_keep, uint32_t key) {
  __shared__ float red[16];
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const bf16_t* xr = x + (long)(row_idx ? row_idx[r] : r) * ldx;
    float ss = 0.f;
    for (int c = threadIdx.x * 8; c < d; c += 256 * 8) {
      float f[8];
      unpack8(*(const uint4*)(xr + c), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += f[j] * f[j];
    }
    ss = block_sum(ss, red);
    const float rs = rsqrtf(ss / (float)d + eps);
    if (rstd_out && threadIdx.x == 0) rstd_out[r] = rs;
    for (int c = threadIdx.x * 8; c < d; c += 256 * 8) {
      float f[8], g[8];
      unpack8(*(const uint4*)(xr + c), f);
      unpack8(*(const uint4*)(w + c), g);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = f[j] * rs * g[j];
      const uint4 pk = pack8(f);
      *(uint4*)(y + (long)r * ldy + c) = pk;
      if (DROP) *(uint4*)(yd + (long)r * d + c) = dropout_chunk(pk, ((long)r * d + c) >> 3, thresh16, inv_keep, key);
    }
  }
}

#define RMS_MAX_ITERS 4
// The decoder's residual stream in fp32 (RV_RESID_FP32=1, opt-in, round 5: the stream's 64 bf16 roundings are 43 % of the per-token
// log-prob error variance).  The projection GEMMs keep writing their BRANCH output in bf16 (o_proj / down_proj
// without the residual operand: the rounding is relative to the small branch, not to the large stream); this kernel adds the branch to
// the fp32 stream and normalises the sum in one pass:   xout = x + add (fp32, ADD only);   y = rmsnorm(xout or x) * w (bf16).
// The row's values stay in registers between the two passes (d <= 8192).
template <bool ADD>
__global__ __launch_bounds__(256) void rmsnorm_fwd_f32_kernel(const float* __restrict__ x, long ldx,
                                                              const int* __restrict__ row_idx,
                                                              const bf16_t* __restrict__ add, long ldadd,
                                                              float* __restrict__ xout, long ldxout,
                                                              const bf16_t* __restrict__ w, bf16_t* __restrict__ y, long ldy,
                                                              float* __restrict__ rstd_out, int rows, int d, float eps) {
  __shared__ float red[16];
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const long xrow = row_idx ? row_idx[r] : r;
    const float* xr = x + xrow * ldx;
    float v[RMS_MAX_ITERS][8];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < RMS_MAX_ITERS; ++i) {
      const int c = threadIdx.x * 8 + i * 2048;
      if (c < d) {
        ln_load8(xr + c, v[i]);
        if (ADD) {
          float a[8];
          unpack8(*(const uint4*)(add + xrow * ldadd + c), a);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[i][j] += a[j];
          float* o = xout + xrow * ldxout + c;
          *(float4*)o = make_float4(v[i][0], v[i][1], v[i][2], v[i][3]);
          *(float4*)(o + 4) = make_float4(v[i][4], v[i][5], v[i][6], v[i][7]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += v[i][j] * v[i][j];
      }
    }
    ss = block_sum(ss, red);
    const float rs = rsqrtf(ss / (float)d + eps);
    if (rstd_out && threadIdx.x == 0) rstd_out[r] = rs;
    if (y) {
#pragma unroll
      for (int i = 0; i < RMS_MAX_ITERS; ++i) {
        const int c = threadIdx.x * 8 + i * 2048;
        if (c < d) {
          float g[8], f[8];
          unpack8(*(const uint4*)(w + c), g);
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] = v[i][j] * rs * g[j];
          *(uint4*)(y + (long)r * ldy + c) = pack8(f);
        }
      }
    }
  }
}

// out (fp32) = x (fp32) + b (bf16): the last branch of the stack joins the fp32 stream (no norm follows it in the layer loop)
__global__ void add_f32_bf16_kernel(const float* __restrict__ x, const bf16_t* __restrict__ b, float* __restrict__ out, long n8) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    float f[8], a[8];
    ln_load8(x + 8 * i, f);
    unpack8(((const uint4*)b)[i], a);
    *(float4*)(out + 8 * i) = make_float4(f[0] + a[0], f[1] + a[1], f[2] + a[2], f[3] + a[3]);
    *(float4*)(out + 8 * i + 4) = make_float4(f[4] + a[4], f[5] + a[5], f[6] + a[6], f[7] + a[7]);
  }
}

// dx = rstd * (g - xhat * mean(g * xhat)) [+ dres], g = dy * w;  dw_partial[block] += dy * xhat
template <typename XT>      // XT = float: the fp32 residual stream (RV_RESID_FP32); gradients stay bf16
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(const bf16_t* __restrict__ dy, long lddy,
                                                          const XT* __restrict__ x, long ldx,
                                                          const int* __restrict__ row_idx,
                                                          const bf16_t* __restrict__ w,
                                                          const float* __restrict__ rstd,
                                                          const bf16_t* __restrict__ dres, long lddres,
                                                          bf16_t* __restrict__ dx, long lddx,
                                                          float* __restrict__ dw_partial, int rows, int d) {
  __shared__ float red[16];
  float dwacc[RMS_MAX_ITERS][8];
#pragma unroll
  for (int i = 0; i < RMS_MAX_ITERS; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) dwacc[i][j] = 0.f;
  const int rows_per = (rows + gridDim.x - 1) / gridDim.x;
  const int r0 = blockIdx.x * rows_per, r1 = min(rows, r0 + rows_per);
  for (int r = r0; r < r1; ++r) {
    const long xrow = row_idx ? row_idx[r] : r;
    const XT* xr = x + xrow * ldx;
    const bf16_t* dyr = dy + (long)r * lddy;
    const float rs = rstd[r];
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < RMS_MAX_ITERS; ++i) {
      const int c = threadIdx.x * 8 + i * 2048;
      if (c < d) {
        float fx[8], fy[8], fw[8];
        ln_load8(xr + c, fx);
        unpack8(*(const uint4*)(dyr + c), fy);
        unpack8(*(const uint4*)(w + c), fw);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float xh = fx[j] * rs;
          dot += fy[j] * fw[j] * xh;
          dwacc[i][j] += fy[j] * xh;
        }
      }
    }
    dot = block_sum(dot, red) / (float)d;
    bf16_t* dxr = dx + xrow * lddx;
#pragma unroll
    for (int i = 0; i < RMS_MAX_ITERS; ++i) {
      const int c = threadIdx.x * 8 + i * 2048;
      if (c < d) {
        float fx[8], fy[8], fw[8], o[8];
        ln_load8(xr + c, fx);
        unpack8(*(const uint4*)(dyr + c), fy);
        unpack8(*(const uint4*)(w + c), fw);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = rs * (fy[j] * fw[j] - fx[j] * rs * dot);
        if (dres) {
          float fr[8];
          unpack8(*(const uint4*)(dres + xrow * lddres + c), fr);
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] += fr[j];
        }
        *(uint4*)(dxr + c) = pack8(o);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < RMS_MAX_ITERS; ++i) {
    const int c = threadIdx.x * 8 + i * 2048;
    if (c < d) {
#pragma unroll
      for (int j = 0; j < 8; ++j) dw_partial[(long)blockIdx.x * d + c + j] = dwacc[i][j];
    }
  }
}

// out[c] (bf16) = sum_p partial[p][c]  (+ existing out if accumulate), c < d; rows of `partial` are `ldp` floats apart (ldp >= d:
// the LayerNorm backward keeps two d-wide halves in one row).  Block = 32 columns x 8 partial slices
// (fixed summation order -> deterministic); grid = d / 32 blocks instead of d / 256 single-column walkers.
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ partial, int nparts, int d, int ldp,
                                                              bf16_t* __restrict__ out, int accumulate) {
  __shared__ float red[8][33];
  const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  float s = 0.f;
  if (c < d)
    for (int p = sl; p < nparts; p += 8) s += partial[(long)p * ldp + c];
  red[sl][cl] = s;
  __syncthreads();
  if (sl == 0 && c < d) {
    float t = accumulate ? bf2f(out[c]) : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) t += red[i][cl];
    out[c] = f2bf(t);
  }
}

// ------------------------------------------------------------------ LayerNorm (CLIP, forward only)
// XT = bf16_t: the tower's bf16 residual stream; XT = float: the fp32 residual stream of RV_CLIP_FP32_RESID (round 5: the frozen tower's
// residual stream carried in fp32 - 84 % of the vision front's share of the per-token error, DESIGN section 2 - output stays bf16)
template <typename XT>
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const XT* __restrict__ x, long ldx,
                                                            const bf16_t* __restrict__ w,
                                                            const bf16_t* __restrict__ b, bf16_t* __restrict__ y,
                                                            long ldy, int rows, int d, float eps) {
  __shared__ float red[16];
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const XT* xr = x + (long)r * ldx;
    float s = 0.f;
    for (int c = threadIdx.x * 8; c < d; c += 2048) {
      float f[8];
      ln_load8(xr + c, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) s += f[j];
    }
    const float mean = block_sum(s, red) / (float)d;
    float v = 0.f;
    for (int c = threadIdx.x * 8; c < d; c += 2048) {
      float f[8];
      ln_load8(xr + c, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) v += (f[j] - mean) * (f[j] - mean);
    }
    const float rs = rsqrtf(block_sum(v, red) / (float)d + eps);
    for (int c = threadIdx.x * 8; c < d; c += 2048) {
      float f[8], g[8], h[8];
      ln_load8(xr + c, f);
      unpack8(*(const uint4*)(w + c), g);
      unpack8(*(const uint4*)(b + c), h);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = (f[j] - mean) * rs * g[j] + h[j];
      *(uint4*)(y + (long)r * ldy + c) = pack8(f);
    }
  }
}


// LayerNorm backward (the OmniLMM Resampler's ln_q / ln_kv / ln_post are trainable: omnilmm/model/resampler.py:127-129).
// mean / rstd are recomputed from x (one extra pass over a row that is in cache anyway) instead of being stored by the
// forward; dgamma / dbeta go through the same fixed-order two-stage reduction as the RMSNorm gain gradient.
// x rows may repeat with period `period` (rows r and r + period share one x row: the learned queries, identical for every image).
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const bf16_t* __restrict__ dy, long lddy,
                                                            const bf16_t* __restrict__ x, long ldx, int period,
                                                            const bf16_t* __restrict__ w, bf16_t* __restrict__ dx, long lddx,
                                                            float* __restrict__ partial, int rows, int d, float eps) {
  __shared__ float red[16];
  float gacc[RMS_MAX_ITERS][8], bacc[RMS_MAX_ITERS][8];
#pragma unroll
  for (int i = 0; i < RMS_MAX_ITERS; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) gacc[i][j] = bacc[i][j] = 0.f;
  const int rows_per = (rows + gridDim.x - 1) / gridDim.x;
  const int r0 = blockIdx.x * rows_per, r1 = min(rows, r0 + rows_per);
  for (int r = r0; r < r1; ++r) {
    const bf16_t* xr = x + (long)(period > 0 ? r % period : r) * ldx;
    const bf16_t* dyr = dy + (long)r * lddy;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < RMS_MAX_ITERS; ++i) {
      const int c = threadIdx.x * 8 + i * 2048;
      if (c < d) {
        float f[8];
        unpack8(*(const uint4*)(xr + c), f);
#pragma unroll
        for (int j = 0; j < 8; ++j) s += f[j];
      }
    }
    const float mean = block_sum(s, red) / (float)d;
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < RMS_MAX_ITERS; ++i) {
      const int c = threadIdx.x * 8 + i * 2048;
      if (c < d) {
        float f[8];
        unpack8(*(const uint4*)(xr + c), f);
#pragma unroll
        for (int j = 0; j < 8; ++j) v += (f[j] - mean) * (f[j] - mean);
      }
    }
    const float rs = rsqrtf(block_sum(v, red) / (float)d + eps);
    float s1 = 0.f, s2 = 0.f;        // sum(dy*w), sum(dy*w*xhat)
#pragma unroll
    for (int i = 0; i < RMS_MAX_ITERS; ++i) {
      const int c = threadIdx.x * 8 + i * 2048;
      if (c < d) {
        float fx[8], fy[8], fw[8];
        unpack8(*(const uint4*)(xr + c), fx);
        unpack8(*(const uint4*)(dyr + c), fy);
        unpack8(*(const uint4*)(w + c), fw);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float xh = (fx[j] - mean) * rs, g = fy[j] * fw[j];
          s1 += g;
          s2 += g * xh;
          gacc[i][j] += fy[j] * xh;
          bacc[i][j] += fy[j];
        }
      }
    }
    s1 = block_sum(s1, red) / (float)d;
    s2 = block_sum(s2, red) / (float)d;
    if (dx) {
      bf16_t* dxr = dx + (long)r * lddx;
#pragma unroll
      for (int i = 0; i < RMS_MAX_ITERS; ++i) {
        const int c = threadIdx.x * 8 + i * 2048;
        if (c < d) {
          float fx[8], fy[8], fw[8], o[8];
          unpack8(*(const uint4*)(xr + c), fx);
          unpack8(*(const uint4*)(dyr + c), fy);
          unpack8(*(const uint4*)(w + c), fw);
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = rs * (fy[j] * fw[j] - s1 - (fx[j] - mean) * rs * s2);
          *(uint4*)(dxr + c) = pack8(o);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < RMS_MAX_ITERS; ++i) {
    const int c = threadIdx.x * 8 + i * 2048;
    if (c < d) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        partial[(long)blockIdx.x * 2 * d + c + j] = gacc[i][j];
        partial[(long)blockIdx.x * 2 * d + d + c + j] = bacc[i][j];
      }
    }
  }
}

// y[r][:] = x[r][:] + p[r % period][:]   (position tables broadcast over the images of a batch)
__global__ __launch_bounds__(256) void add_rows_kernel(const bf16_t* __restrict__ x, long ldx, const bf16_t* __restrict__ p,
                                                       long ldp, int period, bf16_t* __restrict__ y, long ldy, long rows,
                                                       int d) {
  const int cpr = d >> 3;
  const long total = rows * cpr;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / cpr;
    const int c = (int)(i % cpr) * 8;
    float a[8], b[8];
    unpack8(*(const uint4*)(x + r * ldx + c), a);
    unpack8(*(const uint4*)(p + (r % period) * ldp + c), b);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] += b[j];
    *(uint4*)(y + r * ldy + c) = pack8(a);
  }
}

// y[q][:] = sum_b x[b * period + q][:]  (fp32 accumulation in fixed order b = 0, 1, ...: deterministic)
__global__ __launch_bounds__(256) void sum_rows_periodic_kernel(const bf16_t* __restrict__ x, long ldx, int period, int reps,
                                                                bf16_t* __restrict__ y, long ldy, int d) {
  const int cpr = d >> 3;
  const long total = (long)period * cpr;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long q = i / cpr;
    const int c = (int)(i % cpr) * 8;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < reps; ++b) {
      float a[8];
      unpack8(*(const uint4*)(x + ((long)b * period + q) * ldx + c), a);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += a[j];
    }
    *(uint4*)(y + q * ldy + c) = pack8(acc);
  }
}

// ------------------------------------------------------------------ RoPE (half-split layout), in place
// x: [n_tok][ld]; rotates `n_heads_total` heads of width hd starting at column 0 (q then k are adjacent).
__global__ void rope_kernel(bf16_t* __restrict__ x, long ld, const float* __restrict__ cs_cos,
                            const float* __restrict__ cs_sin, const int* __restrict__ pos_tab, long n_tok, int L,
                            int n_heads_total, int hd, float sign) {
  const int half = hd >> 1, cpr = half >> 3;  // 16-byte chunks per half head
  const long total = n_tok * n_heads_total * cpr;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ch = (int)(i % cpr);
    const long t2 = i / cpr;
    const int h = (int)(t2 % n_heads_total);
    const long n = t2 / n_heads_total;
    const int pos = pos_tab ? pos_tab[n] : (int)(n % L);
    bf16_t* p1 = x + n * ld + (long)h * hd + ch * 8;
    bf16_t* p2 = p1 + half;
    float a[8], b[8], o1[8], o2[8];
    unpack8(*(const uint4*)p1, a);
    unpack8(*(const uint4*)p2, b);
    const float* c = cs_cos + (long)pos * half + ch * 8;
    const float* s = cs_sin + (long)pos * half + ch * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float cc = c[j], ss = s[j] * sign;
      o1[j] = a[j] * cc - b[j] * ss;
      o2[j] = b[j] * cc + a[j] * ss;
    }
    *(uint4*)p1 = pack8(o1);
    *(uint4*)p2 = pack8(o2);
  }
}

// ------------------------------------------------------------------ SwiGLU
// IL = 0: gu = [gate (f columns) | up (f columns)] per row;  IL = 1: interleaved (column 2j = gate_j, 2j+1 = up_j) - the
// layout of the fused gate|up weight whose GEMM epilogue computes SwiGLU itself (EpiSwiGLU); this kernel then only serves the
// recompute paths (activation checkpointing, RV_KEEP_RECOMPUTABLE=0).
// DROP: also writes actd = rv_dropout(act) (contiguous [rows][f]) - the LoRA branch input of the down projection
template <int IL, bool DROP = false>
__global__ void swiglu_fwd_kernel(const bf16_t* __restrict__ gu, long ldgu, bf16_t* __restrict__ act, long lda,
                                  long rows, int f, bf16_t* __restrict__ actd = nullptr, uint32_t thresh16 = 0,
                                  float inv_keep = 1.f, uint32_t key = 0) {
  const int cpr = f >> 3;
  const long total = rows * cpr;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / cpr;
    const int c = (int)(i % cpr) * 8;
    float g[8], u[8], o[8];
    if (IL) {
      float a[8], b[8];
      unpack8(*(const uint4*)(gu + r * ldgu + 2 * c), a);
      unpack8(*(const uint4*)(gu + r * ldgu + 2 * c + 8), b);
#pragma unroll
      for (int j = 0; j < 4; ++j) { g[j] = a[2 * j]; u[j] = a[2 * j + 1]; g[4 + j] = b[2 * j]; u[4 + j] = b[2 * j + 1]; }
    } else {
      unpack8(*(const uint4*)(gu + r * ldgu + c), g);
      unpack8(*(const uint4*)(gu + r * ldgu + f + c), u);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = g[j] / (1.f + __expf(-g[j])) * u[j];
    const uint4 pk = pack8(o);
    *(uint4*)(act + r * lda + c) = pk;
    if (DROP) *(uint4*)(actd + r * f + c) = dropout_chunk(pk, i, thresh16, inv_keep, key);      // i = (r * f + c) / 8
  }
}

template <int IL>
__global__ void swiglu_bwd_kernel(const bf16_t* __restrict__ dact, long ldd, const bf16_t* __restrict__ gu,
                                  long ldgu, bf16_t* __restrict__ dgu, long lddgu, long rows, int f) {
  const int cpr = f >> 3;
  const long total = rows * cpr;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / cpr;
    const int c = (int)(i % cpr) * 8;
    float g[8], u[8], da[8], dg[8], du[8];
    if (IL) {
      float a[8], b[8];
      unpack8(*(const uint4*)(gu + r * ldgu + 2 * c), a);
      unpack8(*(const uint4*)(gu + r * ldgu + 2 * c + 8), b);
#pragma unroll
      for (int j = 0; j < 4; ++j) { g[j] = a[2 * j]; u[j] = a[2 * j + 1]; g[4 + j] = b[2 * j]; u[4 + j] = b[2 * j + 1]; }
    } else {
      unpack8(*(const uint4*)(gu + r * ldgu + c), g);
      unpack8(*(const uint4*)(gu + r * ldgu + f + c), u);
    }
    unpack8(*(const uint4*)(dact + r * ldd + c), da);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float sg = 1.f / (1.f + __expf(-g[j]));
      const float silu = g[j] * sg;
      dg[j] = da[j] * u[j] * sg * (1.f + g[j] * (1.f - sg));
      du[j] = da[j] * silu;
    }
    if (IL) {
      float a[8], b[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) { a[2 * j] = dg[j]; a[2 * j + 1] = du[j]; b[2 * j] = dg[4 + j]; b[2 * j + 1] = du[4 + j]; }
      *(uint4*)(dgu + r * lddgu + 2 * c) = pack8(a);
      *(uint4*)(dgu + r * lddgu + 2 * c + 8) = pack8(b);
    } else {
      *(uint4*)(dgu + r * lddgu + c) = pack8(dg);
      *(uint4*)(dgu + r * lddgu + f + c) = pack8(du);
    }
  }
}

// ------------------------------------------------------------------ dropout on the LoRA branch (peft lora_dropout)
// Counter-based mask: element e of a launch is kept iff its 16 hash bits (mix32 of the element-pair index and a seed-derived key) >= p * 2^16, so the backward
// pass regenerates the identical mask from (seed, e) and nothing is stored.  y = keep ? x / (1 - p) : 0.
__global__ void dropout_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, bf16_t* __restrict__ acc, long n8,
                               uint32_t thresh16, float inv_keep, uint32_t key) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    float f[8];
    unpack8(((const uint4*)x)[i], f);
    // one 32-bit hash serves two elements (16 random bits each: p is resolved to 1.5e-5) - the integer multiplies
    // of the mixer, not HBM, bound this kernel otherwise
    const uint32_t base = drop_base((uint32_t)(i >> 30), key);
#pragma unroll
    for (int j = 0; j < 4; ++j) drop_keep2(drop_pair_bits((uint32_t)i * 4u + (uint32_t)j, base), thresh16, inv_keep, f[2 * j], f[2 * j + 1]);
    if (y) ((uint4*)y)[i] = pack8(f);
    if (acc) {
      float a[8];
      unpack8(((const uint4*)acc)[i], a);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] += f[j];
      ((uint4*)acc)[i] = pack8(a);
    }
  }
}

// ------------------------------------------------------------------ CLIP image preprocessing (PIL BICUBIC resize + normalise)
// Pillow's ImagingResampleHorizontal_8bpc / Vertical_8bpc: 22-bit fixed-point taps, accumulator seeded with 1 << 21,
// clip8(acc >> 22) after EACH pass.  Tap tables come from the host (rlaif-v_amd/image.py); only the cropped window is made.
__device__ __forceinline__ int clip8_fixed(int acc) {
  const int v = acc >> 22;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}
// tmp[r][x][c] = clip8(sum_t src[y0 + r][x0(x) + t][c] * kk[x][t]),  r < rows, x < out_w, c < 3
__global__ void resize_h_u8_kernel(const uint8_t* __restrict__ src, int W, int y0, int rows, const int* __restrict__ bounds,
                                   const int* __restrict__ kk, int ksize, int out_w, uint8_t* __restrict__ tmp) {
  const long n = (long)rows * out_w * 3;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    const int c = (int)(e % 3);
    const int x = (int)((e / 3) % out_w);
    const int r = (int)(e / (3L * out_w));
    const int x0 = bounds[2 * x], nt = bounds[2 * x + 1];
    const uint8_t* row = src + ((long)(y0 + r) * W + x0) * 3 + c;
    const int* k = kk + (long)x * ksize;
    int acc = 1 << 21;
    for (int t = 0; t < nt; ++t) acc += (int)row[3 * t] * k[t];
    tmp[e] = (uint8_t)clip8_fixed(acc);
  }
}
// out[c][y][x] = table[c][clip8(sum_t tmp[r0(y) + t][x][c] * kk[y][t])]   (CHW float32: rescale + normalise via table)
__global__ void resize_v_norm_u8_kernel(const uint8_t* __restrict__ tmp, int out_w, const int* __restrict__ bounds,
                                        const int* __restrict__ kk, int ksize, int out_h, const float* __restrict__ table,
                                        float* __restrict__ out) {
  const long n = 3L * out_h * out_w;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    const int x = (int)(e % out_w);
    const int y = (int)((e / out_w) % out_h);
    const int c = (int)(e / ((long)out_w * out_h));
    const int r0 = bounds[2 * y], nt = bounds[2 * y + 1];
    const uint8_t* col = tmp + ((long)r0 * out_w + x) * 3 + c;
    const int* k = kk + (long)y * ksize;
    int acc = 1 << 21;
    for (int t = 0; t < nt; ++t) acc += (int)col[(long)t * out_w * 3] * k[t];
    out[e] = table[c * 256 + clip8_fixed(acc)];
  }
}

// ------------------------------------------------------------------ GELU(erf) for the projector
__global__ void gelu_fwd_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, long n8) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    float f[8];
    unpack8(((const uint4*)x)[i], f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = 0.5f * f[j] * (1.f + erff(f[j] * 0.70710678118654752f));
    ((uint4*)y)[i] = pack8(f);
  }
}
__global__ void gelu_bwd_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                bf16_t* __restrict__ dx, long n8) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    float f[8], g[8];
    unpack8(((const uint4*)x)[i], f);
    unpack8(((const uint4*)dy)[i], g);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float cdf = 0.5f * (1.f + erff(f[j] * 0.70710678118654752f));
      const float pdf = 0.3989422804014327f * __expf(-0.5f * f[j] * f[j]);
      g[j] = g[j] * (cdf + f[j] * pdf);
    }
    ((uint4*)dx)[i] = pack8(g);
  }
}

// ------------------------------------------------------------------ 2-D transpose with zero padding
// in [R][C] (ld_in) -> out [C][ldo], ldo = roundup(R, 64); out[c][r >= R] = 0.   C % 8 == 0.
__global__ __launch_bounds__(256) void transpose_kernel(const bf16_t* __restrict__ in, long ld_in,
                                                        bf16_t* __restrict__ out, long ldo, int R, int C) {
  __shared__ bf16_t tile[64][72];
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ch = threadIdx.x + i * 256;   // 512 chunks of 8
    const int r = ch >> 3, cc = (ch & 7) * 8;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (r0 + r < R && c0 + cc < C) v = *(const uint4*)(in + (long)(r0 + r) * ld_in + c0 + cc);
    *(uint4*)(&tile[r][cc]) = v;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ch = threadIdx.x + i * 256;
    const int c = ch >> 3, rr = (ch & 7) * 8;   // output row c, 8 consecutive source rows
    if (c0 + c < C) {
      bf16_t t[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) t[j] = tile[rr + j][c];
      uint4 v;
      v.x = t[0] | ((uint32_t)t[1] << 16); v.y = t[2] | ((uint32_t)t[3] << 16);
      v.z = t[4] | ((uint32_t)t[5] << 16); v.w = t[6] | ((uint32_t)t[7] << 16);
      *(uint4*)(out + (long)(c0 + c) * ldo + r0 + rr) = v;
    }
  }
}

// ------------------------------------------------------------------ splice (K4)
// src[n] >= 0: embed row; -1: zero pad row; <= -2: image feature row (-2 - src[n])
__global__ void splice_fwd_kernel(const int* __restrict__ src, const bf16_t* __restrict__ embed,
                                  const bf16_t* __restrict__ feats, bf16_t* __restrict__ out, long n_rows, int d) {
  const int cpr = d >> 3;
  const long total = n_rows * cpr;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long n = i / cpr;
    const int c = (int)(i % cpr) * 8;
    const int sidx = src[n];
    uint4 v = make_uint4(0, 0, 0, 0);
    if (sidx >= 0) v = *(const uint4*)(embed + (long)sidx * d + c);
    else if (sidx <= -2) v = *(const uint4*)(feats + (long)(-2 - sidx) * d + c);
    *(uint4*)(out + n * d + c) = v;
  }
}

// Deterministic embedding backward: block u sums dx rows pos_sorted[seg_off[u] .. seg_off[u+1]) in fp32
// and writes row uniq_ids[u] of dW (bf16).  Rows of dW not listed stay as they are (caller zeroes).
__global__ __launch_bounds__(256) void embed_bwd_kernel(const int* __restrict__ uniq_ids,
                                                        const int* __restrict__ seg_off,
                                                        const int* __restrict__ pos_sorted,
                                                        const bf16_t* __restrict__ dx, bf16_t* __restrict__ dW,
                                                        int d) {
  const int u = blockIdx.x;
  const int a = seg_off[u], b = seg_off[u + 1];
  const long row = uniq_ids[u];
  for (int c = threadIdx.x * 8; c < d; c += 2048) {
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = a; k < b; ++k) {
      float f[8];
      unpack8(*(const uint4*)(dx + (long)pos_sorted[k] * d + c), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += f[j];
    }
    *(uint4*)(dW + row * d + c) = pack8(acc);
  }
}

// dfeat[r] = dx[src_a[r]] + dx[src_b[r]]   (index -1 = absent)
__global__ void feat_grad_kernel(const int* __restrict__ src_a, const int* __restrict__ src_b,
                                 const bf16_t* __restrict__ dx, bf16_t* __restrict__ dfeat, long n_rows, int d) {
  const int cpr = d >> 3;
  const long total = n_rows * cpr;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / cpr;
    const int c = (int)(i % cpr) * 8;
    float o[8] = {0, 0, 0, 0, 0, 0, 0, 0}, f[8];
    const int a = src_a[r], b = src_b[r];
    if (a >= 0) {
      unpack8(*(const uint4*)(dx + (long)a * d + c), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] += f[j];
    }
    if (b >= 0) {
      unpack8(*(const uint4*)(dx + (long)b * d + c), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] += f[j];
    }
    *(uint4*)(dfeat + r * d + c) = pack8(o);
  }
}

// Row gather / zero-filled scatter of 16-byte chunks: out[r] = in[idx[r]]  /  out[idx[r]] = in[r]
__global__ void gather_rows_kernel(const bf16_t* __restrict__ in, long ld_in, const int* __restrict__ idx,
                                   bf16_t* __restrict__ out, long ld_out, long n_rows, int d, int scatter) {
  const int cpr = d >> 3;
  const long total = n_rows * cpr;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / cpr;
    const int c = (int)(i % cpr) * 8;
    const long k = idx[r];
    if (scatter) *(uint4*)(out + k * ld_out + c) = *(const uint4*)(in + r * ld_in + c);
    else *(uint4*)(out + r * ld_out + c) = *(const uint4*)(in + k * ld_in + c);
  }
}

// column sums: db[c] = sum_m dy[m][c]   (bias gradients; bf16 out).  One workgroup per 64 columns: 16 row lanes x 64 column
// lanes (a row slice = one 128-byte line), every thread sums rows ty, ty + 16, ..., then the 16 partial sums of a column are
// added in fixed order (deterministic).  (Round 3: the first version walked all M rows in ONE thread per column - 16
// workgroups, 1.08 ms for the projector's 4608 x 4096 bias gradient; now ~25 us.)
__global__ __launch_bounds__(1024) void colsum_kernel(const bf16_t* __restrict__ dy, long ld, bf16_t* __restrict__ db, int M,
                                                       int N) {
  __shared__ float part[16][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + tx;
  float s = 0.f;
  if (c < N)
    for (int m = ty; m < M; m += 16) s += bf2f(dy[(long)m * ld + c]);
  part[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && c < N) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += part[i][tx];
    db[c] = f2bf(t);
  }
}

// ------------------------------------------------------------------ CLIP front end
// pixels fp32 [B][3][H][W] -> patches bf16 [B*P][Kp], column = c*ps*ps + ky*ps + kx, zero for col >= 3*ps*ps
__global__ void im2col_kernel(const float* __restrict__ px, bf16_t* __restrict__ out, int B, int HW, int ps, int Kp) {
  const int g = HW / ps, P = g * g, K = 3 * ps * ps;
  const long total = (long)B * P * Kp;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int col = (int)(i % Kp);
    const long rp = i / Kp;
    const int p = (int)(rp % P), b = (int)(rp / P);
    float v = 0.f;
    if (col < K) {
      const int c = col / (ps * ps), rem = col % (ps * ps), ky = rem / ps, kx = rem % ps;
      const int py = p / g, pxx = p % g;
      v = px[(((long)b * 3 + c) * HW + (py * ps + ky)) * HW + pxx * ps + kx];
    }
    out[i] = f2bf(v);
  }
}

// x[b][0] = cls + pos[0];  x[b][1+p] = patch[b*P+p] + pos[1+p]
__global__ void clip_assemble_kernel(const bf16_t* __restrict__ patch, const bf16_t* __restrict__ cls,
                                     const bf16_t* __restrict__ pos, bf16_t* __restrict__ x, int B, int P, int d) {
  const int cpr = d >> 3;
  const long total = (long)B * (P + 1) * cpr;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % cpr) * 8;
    const long rt = i / cpr;
    const int t = (int)(rt % (P + 1)), b = (int)(rt / (P + 1));
    float a[8], q[8];
    if (t == 0) unpack8(*(const uint4*)(cls + c), a);
    else unpack8(*(const uint4*)(patch + ((long)b * P + t - 1) * d + c), a);
    unpack8(*(const uint4*)(pos + (long)t * d + c), q);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] += q[j];
    *(uint4*)(x + rt * d + c) = pack8(a);
  }
}

// ------------------------------------------------------------------ optimizer
__global__ void sumsq_kernel(const bf16_t* __restrict__ g, long n8, float* __restrict__ partial) {
  __shared__ float red[16];
  float s = 0.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    float f[8];
    unpack8(((const uint4*)g)[i], f);
#pragma unroll
    for (int j = 0; j < 8; ++j) s += f[j] * f[j];
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// The buffer holds pre_scale^-1 times the true gradient (e.g. a SUM over ranks with pre_scale = 1/world).
// out[0] = ||pre_scale * g||, out[1] = pre_scale * min(1, max_norm / (out[0] + 1e-6))  -> the factor AdamW
// multiplies the raw buffer by (clip disabled when max_norm <= 0).
__global__ void gradnorm_finish_kernel(const float* __restrict__ partial, int nparts, float max_norm,
                                       float pre_scale, float* __restrict__ out) {
  __shared__ float red[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) s += partial[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) {
    const float nrm = sqrtf(s) * pre_scale;
    out[0] = nrm;
    out[1] = pre_scale * ((max_norm > 0.f) ? fminf(1.f, max_norm / (nrm + 1e-6f)) : 1.f);
  }
}

// ZeRO-1 (sharded optimizer, dist.ShardedGradReducer): every rank holds the reduced gradient of ITS shard only, so the global norm is
// sum-of-squares per rank -> one-float all-reduce -> clip factor.  out1[0] (+)= sum of the block partials.
__global__ void sumsq_finish_kernel(const float* __restrict__ partial, int nparts, float* __restrict__ out1, int accumulate) {
  __shared__ float red[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) s += partial[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out1[0] = accumulate ? out1[0] + s : s;
}
__global__ void clip_from_sumsq_kernel(const float* __restrict__ sumsq, float max_norm, float pre_scale, float* __restrict__ out) {
  const float nrm = sqrtf(sumsq[0]) * pre_scale;          // same arithmetic as gradnorm_finish_kernel
  out[0] = nrm;
  out[1] = pre_scale * ((max_norm > 0.f) ? fminf(1.f, max_norm / (nrm + 1e-6f)) : 1.f);
}

// Gradient accumulation over micro-batches (HF Trainer --gradient_accumulation_steps): fp32 side buffer.
//   mode 0: acc = g            (first micro-batch: no zeroing pass)
//   mode 1: acc += g           (middle micro-batches)
//   mode 2: g = bf16((acc + g) * scale)   (last micro-batch: the averaged gradient lands where all-reduce / AdamW read it)
__global__ void grad_accum_kernel(float* __restrict__ acc, bf16_t* __restrict__ g, long n8, int mode, float scale) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    float gf[8];
    unpack8(((const uint4*)g)[i], gf);
    if (mode == 0) {
      ((float4*)acc)[2 * i] = make_float4(gf[0], gf[1], gf[2], gf[3]);
      ((float4*)acc)[2 * i + 1] = make_float4(gf[4], gf[5], gf[6], gf[7]);
      continue;
    }
    const float4 a0 = ((const float4*)acc)[2 * i], a1 = ((const float4*)acc)[2 * i + 1];
    float s[8] = {a0.x + gf[0], a0.y + gf[1], a0.z + gf[2], a0.w + gf[3], a1.x + gf[4], a1.y + gf[5], a1.z + gf[6], a1.w + gf[7]};
    if (mode == 1) {
      ((float4*)acc)[2 * i] = make_float4(s[0], s[1], s[2], s[3]);
      ((float4*)acc)[2 * i + 1] = make_float4(s[4], s[5], s[6], s[7]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] *= scale;
      ((uint4*)g)[i] = pack8(s);
    }
  }
}

// AdamW with decoupled weight decay on fp32 master weights; writes the bf16 working copy.
__global__ void adamw_kernel(bf16_t* __restrict__ p, float* __restrict__ master, float* __restrict__ m,
                             float* __restrict__ v, const bf16_t* __restrict__ g, long n8, float lr, float b1,
                             float b2, float eps, float wd, float bc1, float bc2_sqrt,
                             const float* __restrict__ clip) {
  const float gs = clip ? clip[1] : 1.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    float gf[8], o[8];
    unpack8(((const uint4*)g)[i], gf);
    float4 w0 = ((float4*)master)[2 * i], w1 = ((float4*)master)[2 * i + 1];
    float4 m0 = ((float4*)m)[2 * i], m1 = ((float4*)m)[2 * i + 1];
    float4 v0 = ((float4*)v)[2 * i], v1 = ((float4*)v)[2 * i + 1];
    float wf[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    float mf[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
    float vf[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float gg = gf[j] * gs;
      wf[j] *= (1.f - lr * wd);
      mf[j] = b1 * mf[j] + (1.f - b1) * gg;
      vf[j] = b2 * vf[j] + (1.f - b2) * gg * gg;
      const float denom = sqrtf(vf[j]) / bc2_sqrt + eps;
      wf[j] -= (lr / bc1) * (mf[j] / denom);
      o[j] = wf[j];
    }
    ((float4*)master)[2 * i] = make_float4(wf[0], wf[1], wf[2], wf[3]);
    ((float4*)master)[2 * i + 1] = make_float4(wf[4], wf[5], wf[6], wf[7]);
    ((float4*)m)[2 * i] = make_float4(mf[0], mf[1], mf[2], mf[3]);
    ((float4*)m)[2 * i + 1] = make_float4(mf[4], mf[5], mf[6], mf[7]);
    ((float4*)v)[2 * i] = make_float4(vf[0], vf[1], vf[2], vf[3]);
    ((float4*)v)[2 * i + 1] = make_float4(vf[4], vf[5], vf[6], vf[7]);
    ((uint4*)p)[i] = pack8(o);
  }
}

// ------------------------------------------------------------------ log-prob reductions + DPO loss
// lse[m] = log sum_n exp(logit[m][n]) from per-64-column partials; logp[m] = tgt_logit[m] - lse[m]
// One wave per row; every lane returns the row's lse.  Shared by both finish kernels: same operations in the same order.
__device__ __forceinline__ float logp_row_lse(const float* __restrict__ pmax, const float* __restrict__ psum, int nblk, int m,
                                              int lane) {
  float mx = -INFINITY;
  for (int i = lane; i < nblk; i += 64) mx = fmaxf(mx, pmax[(long)m * nblk + i]);
  mx = wave_max(mx);
  float s = 0.f;
  for (int i = lane; i < nblk; i += 64) s += psum[(long)m * nblk + i] * __expf(pmax[(long)m * nblk + i] - mx);
  s = wave_sum(s);
  return mx + logf(s);
}

__global__ void logp_finish_kernel(const float* __restrict__ pmax, const float* __restrict__ psum,
                                   const float* __restrict__ tgt_logit, int nblk, int M,
                                   float* __restrict__ lse, float* __restrict__ logp) {
  const int m = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (m >= M) return;
  const int lane = threadIdx.x & 63;
  const float l = logp_row_lse(pmax, psum, nblk, m, lane);
  if (lane == 0) {
    lse[m] = l;
    logp[m] = tgt_logit[m] - l;
  }
}

// finish + unpack (the packed log-prob precompute): row m's logp goes to its one or two slots of the per-token matrix and to
// its slot of the compact vector of selected rows; a negative index means no such slot.  Every destination has one writer.
__global__ void logp_finish_unpack_kernel(const float* __restrict__ pmax, const float* __restrict__ psum,
                                          const float* __restrict__ tgt_logit, int nblk, int M,
                                          const int* __restrict__ dst_a, const int* __restrict__ dst_b,
                                          const int* __restrict__ dst_c, float* __restrict__ per_token, long n_per_token,
                                          float* __restrict__ compact, int n_compact) {
  const int m = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (m >= M) return;
  const int lane = threadIdx.x & 63;
  const float l = logp_row_lse(pmax, psum, nblk, m, lane);
  if (lane == 0) {
    const float lp = tgt_logit[m] - l;
    const int a = dst_a[m], b = dst_b[m], c = dst_c[m];
    if (a >= 0 && a < n_per_token) per_token[a] = lp;
    if (b >= 0 && b < n_per_token) per_token[b] = lp;
    if (c >= 0 && c < n_compact) compact[c] = lp;
  }
}

// ------------------------------------------------------------------ next-token scores (yes / no feedback scoring)
// One workgroup per row of fp32 logits: softmax over the columns [0, V_valid) after HF's RepetitionPenaltyLogitsProcessor (a logit
// of a token id the prompt contains becomes l / penalty if l > 0, else l * penalty), read at the K wanted ids, plus lse and the
// argmax (lowest index among equal maxima).  The prompt's ids are a bitmap in LDS (V_valid / 8 bytes), so the row is read ONCE
// with an online softmax per thread; the partial (max, sum, argmax) triples are combined in a fixed order: deterministic.
struct NtsPart {
  float mx, sum;
  int idx;
};
__device__ __forceinline__ NtsPart nts_combine(const NtsPart& a, const NtsPart& b) {
  NtsPart r;
  r.mx = fmaxf(a.mx, b.mx);
  r.idx = (b.mx > a.mx || (b.mx == a.mx && b.idx < a.idx)) ? b.idx : a.idx;
  const float fa = (a.mx == -INFINITY) ? 0.f : expf(a.mx - r.mx), fb = (b.mx == -INFINITY) ? 0.f : expf(b.mx - r.mx);
  r.sum = a.sum * fa + b.sum * fb;
  return r;
}
__device__ __forceinline__ float nts_penalised(float l, bool seen, float penalty) {
  return seen ? (l > 0.f ? l / penalty : l * penalty) : l;
}

__global__ __launch_bounds__(256) void next_token_scores_kernel(const float* __restrict__ logits, long ldl, int V_valid,
                                                                const int* __restrict__ seen_off,
                                                                const int* __restrict__ seen_ids, float penalty,
                                                                const int* __restrict__ want_ids, int K,
                                                                float* __restrict__ probs, float* __restrict__ logp,
                                                                int* __restrict__ argmax, float* __restrict__ lse) {
  extern __shared__ uint32_t nts_bits[];          // [ceil(V_valid / 32)] when the penalty is on
  __shared__ NtsPart part[4];
  __shared__ float row_lse;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* row = logits + (long)m * ldl;
  const bool pen = seen_off != nullptr && penalty != 1.0f;
  if (pen) {
    const int nw = (V_valid + 31) >> 5;
    for (int i = tid; i < nw; i += 256) nts_bits[i] = 0u;
    __syncthreads();
    for (int i = seen_off[m] + tid; i < seen_off[m + 1]; i += 256) {
      const int id = seen_ids[i];
      if (id >= 0 && id < V_valid) atomicOr(&nts_bits[id >> 5], 1u << (id & 31));
    }
    __syncthreads();
  }
  auto value = [&](int i) { return nts_penalised(row[i], pen && ((nts_bits[i >> 5] >> (i & 31)) & 1u), penalty); };
  NtsPart a = {-INFINITY, 0.f, 0x7fffffff};
  for (int i = tid; i < V_valid; i += 256) {
    const float l = value(i);
    if (l > a.mx) {                                // indices grow inside a thread: the first of equal maxima stays
      a.sum = (a.mx == -INFINITY ? 0.f : a.sum * expf(a.mx - l)) + 1.f;
      a.mx = l;
      a.idx = i;
    } else if (l != -INFINITY) {
      a.sum += expf(l - a.mx);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    NtsPart b;
    b.mx = __shfl_xor(a.mx, o, 64);
    b.sum = __shfl_xor(a.sum, o, 64);
    b.idx = __shfl_xor(a.idx, o, 64);
    a = (lane & o) ? nts_combine(b, a) : nts_combine(a, b);      // both lanes of a pair evaluate the same expression
  }
  if (lane == 0) part[wave] = a;
  __syncthreads();
  if (tid == 0) {
    NtsPart r = nts_combine(nts_combine(part[0], part[1]), nts_combine(part[2], part[3]));
    row_lse = r.mx + logf(r.sum);
    lse[m] = row_lse;
    argmax[m] = r.idx;
  }
  __syncthreads();
  for (int k = tid; k < K; k += 256) {
    const int id = want_ids[k];
    const float lp = (id >= 0 && id < V_valid) ? value(id) - row_lse : -INFINITY;
    logp[(long)m * K + k] = lp;
    probs[(long)m * K + k] = expf(lp);
  }
}

// per sequence: sum of its selected rows' logp (rows of sequence s are seq_off[s]..seq_off[s+1]),
// fixed summation order -> deterministic.   out_sum[s], out_cnt[s]
__global__ void seq_sum_kernel(const float* __restrict__ logp, const float* __restrict__ weight,
                               const int* __restrict__ seq_off, float* __restrict__ out_sum,
                               float* __restrict__ out_cnt) {
  __shared__ float red[16];
  const int s = blockIdx.x, a = seq_off[s], b = seq_off[s + 1];
  float acc = 0.f, cnt = 0.f;
  for (int i = a + threadIdx.x; i < b; i += blockDim.x) {
    const float w = weight ? weight[i] : 1.f;
    acc += logp[i] * w;
    cnt += w;
  }
  acc = block_sum(acc, red);
  cnt = block_sum(cnt, red);
  if (threadIdx.x == 0) { out_sum[s] = acc; out_cnt[s] = cnt; }
}

// DPO loss (muffin/train/trainers.py:91-126, :297-301) on B pairs, single block.
//   in : seq_sum[2B], seq_cnt[2B] (wins then rejects), ref_win[B], ref_rej[B]
//   out: per_pair[5][B] = losses, chosen_rewards, rejected_rewards, policy_win, policy_rej
//        scalars[8]   = loss, mean chosen reward, mean rejected reward, accuracy, margin, mean win logp, mean rej logp, 0
//        coef[2B]     = dLoss / d seq_sum  (already divided by count when use_average)
__global__ void dpo_loss_kernel(const float* __restrict__ seq_sum, const float* __restrict__ seq_cnt,
                                const float* __restrict__ ref_win, const float* __restrict__ ref_rej, int B,
                                float beta, int use_average, float sft_w, float dpo_w,
                                float* __restrict__ per_pair, float* __restrict__ scalars,
                                float* __restrict__ coef) {
  __shared__ float red[16];
  float a_loss = 0, a_cw = 0, a_cr = 0, a_acc = 0, a_pw = 0, a_pr = 0;
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    float pw = seq_sum[i], pr = seq_sum[B + i];
    const float cw_n = seq_cnt[i], cr_n = seq_cnt[B + i];
    if (use_average) { pw = pw / cw_n; pr = pr / cr_n; }
    const float z = (pw - pr) - (ref_win[i] - ref_rej[i]);
    const float bz = beta * z;
    // -logsigmoid(bz) = softplus(-bz), stable form
    const float loss = fmaxf(-bz, 0.f) + log1pf(__expf(-fabsf(bz)));
    const float sig_neg = 1.f / (1.f + __expf(bz));   // sigmoid(-bz)
    const float cw = beta * (pw - ref_win[i]), cr = beta * (pr - ref_rej[i]);
    per_pair[0 * B + i] = loss; per_pair[1 * B + i] = cw; per_pair[2 * B + i] = cr;
    per_pair[3 * B + i] = pw; per_pair[4 * B + i] = pr;
    float gw = (-dpo_w * beta * sig_neg - sft_w) / (float)B;
    float gr = (dpo_w * beta * sig_neg) / (float)B;
    if (use_average) { gw /= cw_n; gr /= cr_n; }
    coef[i] = gw; coef[B + i] = gr;
    a_loss += loss; a_cw += cw; a_cr += cr; a_acc += (cw > cr) ? 1.f : 0.f; a_pw += pw; a_pr += pr;
  }
  a_loss = block_sum(a_loss, red); a_cw = block_sum(a_cw, red); a_cr = block_sum(a_cr, red);
  a_acc = block_sum(a_acc, red); a_pw = block_sum(a_pw, red); a_pr = block_sum(a_pr, red);
  if (threadIdx.x == 0) {
    const float inv = 1.f / (float)B;
    scalars[0] = dpo_w * a_loss * inv - sft_w * a_pw * inv;
    scalars[1] = a_cw * inv; scalars[2] = a_cr * inv; scalars[3] = a_acc * inv;
    scalars[4] = (a_cw - a_cr) * inv; scalars[5] = a_pw * inv; scalars[6] = a_pr * inv; scalars[7] = 0.f;
  }
}

// row_coef[i] = coef[seq_of_row[i]] * (weight ? weight[i] : 1)
__global__ void row_coef_kernel(const float* __restrict__ coef, const int* __restrict__ seq_of_row,
                                const float* __restrict__ weight, float* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = coef[seq_of_row[i]] * (weight ? weight[i] : 1.f);
}

// delta[(s*H+h)*L + l] = sum_e dO[n][h*hd+e] * O[n][h*hd+e]     (one wave per (n,h))
__global__ __launch_bounds__(256) void attn_delta_kernel(const bf16_t* __restrict__ dO, long lddo,
                                                         const bf16_t* __restrict__ O, long ldo,
                                                         float* __restrict__ delta, int S, int L, int H, int hd) {
  const long total = (long)S * L * H;
  const int lane = threadIdx.x & 63;
  for (long w = blockIdx.x * 4L + (threadIdx.x >> 6); w < total; w += gridDim.x * 4L) {
    const int h = (int)(w % H);
    const long n = w / H;
    float acc = 0.f;
    for (int e = lane * 2; e < hd; e += 128) {
      const uint32_t a = *(const uint32_t*)(dO + n * lddo + (long)h * hd + e);
      const uint32_t b = *(const uint32_t*)(O + n * ldo + (long)h * hd + e);
      acc += bf2f((bf16_t)(a & 0xffff)) * bf2f((bf16_t)(b & 0xffff)) + bf2f((bf16_t)(a >> 16)) * bf2f((bf16_t)(b >> 16));
    }
    acc = wave_sum(acc);
    if (lane == 0) {
      const int s = (int)(n / L), l = (int)(n % L);
      delta[((long)s * H + h) * L + l] = acc;
    }
  }
}

// fp32 -> bf16 and bf16 -> fp32 casts (parameter initialisation plumbing)
__global__ void cast_f32_bf16_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    out[i] = f2bf(in[i]);
}
__global__ void cast_bf16_f32_kernel(const bf16_t* __restrict__ in, float* __restrict__ out, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    out[i] = bf2f(in[i]);
}

inline int grid_for(long work, int block, int cap = 4096) {
  long g = (work + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

}  // namespace

// A gradient exchange seen from ONE GPU: `n_wg` persistent 256-thread workgroups (the footprint of n_wg RCCL channels -
// one CU each, for as long as the bucket lasts) stream  dst[i] = a[i] + b[i]  (the receive-reduce-send of a ring step:
// two 16-byte loads and one 16-byte store per 8 gradients).  bench.py launches it on a side stream at every
// on_bucket_ready to measure what CUs lent to communication cost the backward GEMMs on a single GPU, where no xGMI
// peer exists; it is not on the training path.
__global__ __launch_bounds__(256) void reduce_copy_persistent_kernel(const u32x4_t* __restrict__ a,
                                                                      const u32x4_t* __restrict__ b,
                                                                      u32x4_t* __restrict__ dst, long n16) {
  const long stride = (long)gridDim.x * 256 * 4;
  for (long i0 = (long)blockIdx.x * 256 * 4 + threadIdx.x; i0 < n16; i0 += stride) {
    u32x4_t va[4], vb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long i = i0 + u * 256;
      if (i < n16) {
        va[u] = a[i];
        vb[u] = b[i];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long i = i0 + u * 256;
      if (i < n16) {
        u32x4_t r;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float lo = bf2f((bf16_t)(va[u][j] & 0xffffu)) + bf2f((bf16_t)(vb[u][j] & 0xffffu));
          const float hi = bf2f((bf16_t)(va[u][j] >> 16)) + bf2f((bf16_t)(vb[u][j] >> 16));
          r[j] = pack2bf(lo, hi);
        }
        dst[i] = r;
      }
    }
  }
}

// ---- launch geometry and the launches that several entry points share ----
// one workgroup per row, at most 8192 of them (the kernels stride over the rows)
static dim3 row_grid(int rows) { return dim3(min(rows, 8192)); }

// out[j] (+)= sum over the nb rows of partial[.][j], j < d; the rows are ldp floats apart
static int launch_reduce_partials(const float* partial, int nb, int d, int ldp, void* out, int accumulate, void* stream) {
  return launch<reduce_partials_kernel>(0, dim3((d + 31) / 32), dim3(256), stream, partial, nb, d, ldp, (bf16_t*)out, accumulate);
}

// Kernel(tensors..., work) over a flat range of `work` items, one per thread: the GELU pair (work = n / 8) and the casts
template <auto Kernel, class... T>
static int launch_flat(long work, int cap, void* stream, T... tensors) {
  if (work == 0) return 0;
  return launch<Kernel>(0, dim3(grid_for(work, 256, cap)), dim3(256), stream, tensors..., work);
}

// rv_rmsnorm_bwd (XT = bf16_t) and rv_rmsnorm_bwd_f32x (XT = float), after their own argument checks
template <typename XT>
static int rmsnorm_bwd(const void* dy, long lddy, const XT* x, long ldx, const int* row_idx, const void* w, const float* rstd,
                       const void* dres, long lddres, void* dx, long lddx, float* dw_partial, void* dw, int dw_accumulate, int rows,
                       int d, void* stream) {
  if (rows == 0) return 0;
  const int nb = rv_rmsnorm_bwd_nblocks(rows);
  if (const int rc = launch<rmsnorm_bwd_kernel<XT>>(0, dim3(nb), dim3(256), stream, (const bf16_t*)dy, lddy, x, ldx, row_idx, (const bf16_t*)w,
                                                    rstd, (const bf16_t*)dres, lddres, (bf16_t*)dx, lddx, dw_partial, rows, d))
    return rc;
  return launch_reduce_partials(dw_partial, nb, d, d, dw, dw_accumulate, stream);
}

// rv_layernorm_fwd (XT = bf16_t) and rv_layernorm_fwd_f32in (XT = float), after their own argument checks
template <typename XT>
static int layernorm_fwd(const XT* x, long ldx, const void* w, const void* b, void* y, long ldy, int rows, int d, float eps,
                         void* stream) {
  if (rows == 0) return 0;
  return launch<layernorm_fwd_kernel<XT>>(0, row_grid(rows), dim3(256), stream, x, ldx, (const bf16_t*)w, (const bf16_t*)b, (bf16_t*)y, ldy,
                                          rows, d, eps);
}

// f(std::integral_constant<int, IL>{}): the SwiGLU kernels take the layout (1 = interleaved gate / up columns) as a template argument
template <class F>
static int for_layout(int interleaved, F&& f) {
  return interleaved ? f(std::integral_constant<int, 1>{}) : f(std::integral_constant<int, 0>{});
}

// the first pass of rv_grad_norm and rv_grad_sumsq: partial[1024] = per-workgroup sums of squares
static int launch_sumsq(const void* g, long n, float* partial, void* stream) {
  return launch<sumsq_kernel>(0, dim3(1024), dim3(256), stream, (const bf16_t*)g, n / 8, partial);
}

extern "C" {

int rv_rmsnorm_fwd(const void* x, long ldx, const int* row_idx, const void* w, void* y, long ldy, float* rstd,
                   int rows, int d, float eps, void* stream) {
  RV_REQUIRE(d % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0, "rv_rmsnorm_fwd: d/ld must be multiples of 8");
  if (rows == 0) return 0;
  return launch<rmsnorm_fwd_kernel<false>>(0, row_grid(rows), dim3(256), stream, (const bf16_t*)x, ldx, row_idx, (const bf16_t*)w,
                                           (bf16_t*)y, ldy, rstd, rows, d, eps, (bf16_t*)nullptr, 0u, 1.f, 0u);
}

int rv_rmsnorm_fwd_dropout(const void* x, long ldx, const int* row_idx, const void* w, void* y, long ldy, float* rstd,
                           int rows, int d, float eps, void* yd, float p, int seed, void* stream) {
  RV_REQUIRE(d % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0, "rv_rmsnorm_fwd_dropout: d/ld must be multiples of 8");
  RV_REQUIRE(yd != nullptr && p >= 0.f && p < 1.f, "rv_rmsnorm_fwd_dropout: yd required, 0 <= p < 1");
  if (rows == 0) return 0;
  const DropParams dp = drop_params(p, seed);
  return launch<rmsnorm_fwd_kernel<true>>(0, row_grid(rows), dim3(256), stream, (const bf16_t*)x, ldx, row_idx, (const bf16_t*)w,
                                          (bf16_t*)y, ldy, rstd, rows, d, eps, (bf16_t*)yd, dp.thresh16, dp.inv_keep, dp.key);
}

// workgroups (= fp32 partial rows of dw): 1024 measured best at 27 k rows (512: 278 us, 1024: 239 us, 2048: 296 us, 4096: 377 us - the partial-sum pass grows)
int rv_rmsnorm_bwd_nblocks(int rows) {
  const int cap = 1024;
  return rows < cap ? (rows < 1 ? 1 : rows) : cap;
}

int rv_rmsnorm_bwd(const void* dy, long lddy, const void* x, long ldx, const int* row_idx, const void* w,
                   const float* rstd, const void* dres, long lddres, void* dx, long lddx, float* dw_partial,
                   void* dw, int dw_accumulate, int rows, int d, void* stream) {
  RV_REQUIRE(d % 8 == 0 && d <= 2048 * RMS_MAX_ITERS, "rv_rmsnorm_bwd: d must be a multiple of 8 and <= 8192");
  RV_REQUIRE(lddy % 8 == 0 && ldx % 8 == 0 && lddx % 8 == 0 && lddres % 8 == 0, "rv_rmsnorm_bwd: ld alignment");
  return rmsnorm_bwd(dy, lddy, (const bf16_t*)x, ldx, row_idx, w, rstd, dres, lddres, dx, lddx, dw_partial, dw, dw_accumulate, rows, d, stream);
}

int rv_rmsnorm_bwd_f32x(const void* dy, long lddy, const float* x, long ldx, const int* row_idx, const void* w,
                        const float* rstd, const void* dres, long lddres, void* dx, long lddx, float* dw_partial,
                        void* dw, int dw_accumulate, int rows, int d, void* stream) {
  RV_REQUIRE(d % 8 == 0 && d <= 2048 * RMS_MAX_ITERS, "rv_rmsnorm_bwd_f32x: d must be a multiple of 8 and <= 8192");
  RV_REQUIRE(lddy % 8 == 0 && ldx % 4 == 0 && lddx % 8 == 0 && lddres % 8 == 0, "rv_rmsnorm_bwd_f32x: ld alignment");
  return rmsnorm_bwd(dy, lddy, x, ldx, row_idx, w, rstd, dres, lddres, dx, lddx, dw_partial, dw, dw_accumulate, rows, d, stream);
}

int rv_rmsnorm_fwd_f32(const float* x, long ldx, const int* row_idx, const void* add, long ldadd, float* xout, long ldxout,
                       const void* w, void* y, long ldy, float* rstd, int rows, int d, float eps, void* stream) {
  RV_REQUIRE(d % 8 == 0 && d <= 2048 * RMS_MAX_ITERS && ldx % 4 == 0 && ldy % 8 == 0, "rv_rmsnorm_fwd_f32: d % 8, d <= 8192, ld alignment");
  RV_REQUIRE(add == nullptr || (xout != nullptr && ldadd % 8 == 0 && ldxout % 4 == 0), "rv_rmsnorm_fwd_f32: add needs xout (fp32) and aligned strides");
  RV_REQUIRE(y != nullptr || add != nullptr, "rv_rmsnorm_fwd_f32: nothing to write");
  if (rows == 0) return 0;
  if (add)
    return launch<rmsnorm_fwd_f32_kernel<true>>(0, row_grid(rows), dim3(256), stream, x, ldx, row_idx, (const bf16_t*)add, ldadd, xout, ldxout,
                                                (const bf16_t*)w, (bf16_t*)y, ldy, rstd, rows, d, eps);
  return launch<rmsnorm_fwd_f32_kernel<false>>(0, row_grid(rows), dim3(256), stream, x, ldx, row_idx, (const bf16_t*)nullptr, 0L,
                                               (float*)nullptr, 0L, (const bf16_t*)w, (bf16_t*)y, ldy, rstd, rows, d, eps);
}

int rv_add_f32_bf16(const float* x, const void* b, float* out, long n, void* stream) {
  RV_REQUIRE(n % 8 == 0, "rv_add_f32_bf16: n%8");
  return launch_flat<add_f32_bf16_kernel>(n / 8, 8192, stream, x, (const bf16_t*)b, out);
}

int rv_layernorm_fwd(const void* x, long ldx, const void* w, const void* b, void* y, long ldy, int rows, int d,
                     float eps, void* stream) {
  RV_REQUIRE(d % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0, "rv_layernorm_fwd: alignment");
  return layernorm_fwd((const bf16_t*)x, ldx, w, b, y, ldy, rows, d, eps, stream);
}

int rv_layernorm_fwd_f32in(const float* x, long ldx, const void* w, const void* b, void* y, long ldy, int rows, int d,
                           float eps, void* stream) {
  RV_REQUIRE(d % 8 == 0 && ldx % 4 == 0 && ldy % 8 == 0, "rv_layernorm_fwd_f32in: alignment");
  return layernorm_fwd(x, ldx, w, b, y, ldy, rows, d, eps, stream);
}

int rv_layernorm_bwd(const void* dy, long lddy, const void* x, long ldx, int x_period, const void* w, void* dx, long lddx,
                     float* partial, void* dw, void* db, int accumulate, int rows, int d, float eps, void* stream) {
  RV_REQUIRE(d % 8 == 0 && d <= 2048 * RMS_MAX_ITERS, "rv_layernorm_bwd: d must be a multiple of 8 and <= 8192");
  RV_REQUIRE(lddy % 8 == 0 && ldx % 8 == 0 && lddx % 8 == 0, "rv_layernorm_bwd: ld alignment");
  if (rows == 0) return 0;
  const int nb = rv_rmsnorm_bwd_nblocks(rows);
  if (const int rc = launch<layernorm_bwd_kernel>(0, dim3(nb), dim3(256), stream, (const bf16_t*)dy, lddy, (const bf16_t*)x, ldx, x_period,
                                                  (const bf16_t*)w, (bf16_t*)dx, lddx, partial, rows, d, eps))
    return rc;
  // partial = [nb][2d] (gain | bias halves): each half is reduced over its own d columns, rows 2d floats apart
  if (const int rc = launch_reduce_partials(partial, nb, d, 2 * d, dw, accumulate, stream)) return rc;
  return launch_reduce_partials(partial + d, nb, d, 2 * d, db, accumulate, stream);
}

int rv_add_rows(const void* x, long ldx, const void* p, long ldp, int period, void* y, long ldy, long rows, int d,
                void* stream) {
  RV_REQUIRE(d % 8 == 0 && ldx % 8 == 0 && ldp % 8 == 0 && ldy % 8 == 0 && period > 0, "rv_add_rows: alignment / period");
  if (rows == 0) return 0;
  return launch<add_rows_kernel>(0, dim3(grid_for(rows * (d / 8), 256, 8192)), dim3(256), stream, (const bf16_t*)x, ldx, (const bf16_t*)p,
                                 ldp, period, (bf16_t*)y, ldy, rows, d);
}

int rv_sum_rows_periodic(const void* x, long ldx, int period, int reps, void* y, long ldy, int d, void* stream) {
  RV_REQUIRE(d % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0 && period > 0 && reps > 0, "rv_sum_rows_periodic: alignment");
  return launch<sum_rows_periodic_kernel>(0, dim3(grid_for((long)period * (d / 8), 256, 8192)), dim3(256), stream, (const bf16_t*)x, ldx,
                                          period, reps, (bf16_t*)y, ldy, d);
}

int rv_rope_inplace(void* x, long ld, const float* cos_tab, const float* sin_tab, const int* pos, long n_tok, int L,
                    int n_heads_total, int hd, int backward, void* stream) {
  RV_REQUIRE(hd % 16 == 0 && ld % 8 == 0, "rv_rope_inplace: hd%16, ld%8");
  const long total = n_tok * n_heads_total * (hd / 16);
  if (total == 0) return 0;
  return launch<rope_kernel>(0, dim3(grid_for(total, 256, 16384)), dim3(256), stream, (bf16_t*)x, ld, cos_tab, sin_tab, pos, n_tok, L,
                             n_heads_total, hd, backward ? -1.f : 1.f);
}

int rv_swiglu_fwd(const void* gu, long ldgu, void* act, long lda, long rows, int f, int interleaved, void* stream) {
  RV_REQUIRE(f % 8 == 0 && ldgu % 8 == 0 && lda % 8 == 0, "rv_swiglu_fwd: alignment");
  if (rows == 0) return 0;
  return for_layout(interleaved, [&](auto IL) {
    return launch<swiglu_fwd_kernel<decltype(IL)::value>>(0, dim3(grid_for(rows * (f / 8), 256, 16384)), dim3(256), stream, (const bf16_t*)gu,
                                                          ldgu, (bf16_t*)act, lda, rows, f, (bf16_t*)nullptr, 0u, 1.f, 0u);
  });
}

int rv_swiglu_fwd_dropout(const void* gu, long ldgu, void* act, long lda, long rows, int f, void* actd, float p, int seed,
                          void* stream) {
  RV_REQUIRE(f % 8 == 0 && ldgu % 8 == 0 && lda % 8 == 0, "rv_swiglu_fwd_dropout: alignment");
  RV_REQUIRE(actd != nullptr && p >= 0.f && p < 1.f, "rv_swiglu_fwd_dropout: actd required, 0 <= p < 1");
  if (rows == 0) return 0;
  const DropParams dp = drop_params(p, seed);
  return launch<swiglu_fwd_kernel<0, true>>(0, dim3(grid_for(rows * (f / 8), 256, 16384)), dim3(256), stream, (const bf16_t*)gu, ldgu,
                                            (bf16_t*)act, lda, rows, f, (bf16_t*)actd, dp.thresh16, dp.inv_keep, dp.key);
}

int rv_swiglu_bwd(const void* dact, long ldd, const void* gu, long ldgu, void* dgu, long lddgu, long rows, int f,
                  int interleaved, void* stream) {
  RV_REQUIRE(f % 8 == 0 && ldgu % 8 == 0 && ldd % 8 == 0 && lddgu % 8 == 0, "rv_swiglu_bwd: alignment");
  if (rows == 0) return 0;
  return for_layout(interleaved, [&](auto IL) {
    return launch<swiglu_bwd_kernel<decltype(IL)::value>>(0, dim3(grid_for(rows * (f / 8), 256, 16384)), dim3(256), stream,
                                                          (const bf16_t*)dact, ldd, (const bf16_t*)gu, ldgu, (bf16_t*)dgu, lddgu, rows, f);
  });
}

int rv_gelu_fwd(const void* x, void* y, long n, void* stream) {
  RV_REQUIRE(n % 8 == 0, "rv_gelu_fwd: n%8");
  return launch_flat<gelu_fwd_kernel>(n / 8, 4096, stream, (const bf16_t*)x, (bf16_t*)y);
}
int rv_gelu_bwd(const void* dy, const void* x, void* dx, long n, void* stream) {
  RV_REQUIRE(n % 8 == 0, "rv_gelu_bwd: n%8");
  return launch_flat<gelu_bwd_kernel>(n / 8, 4096, stream, (const bf16_t*)dy, (const bf16_t*)x, (bf16_t*)dx);
}

int rv_dropout(const void* x, void* y, void* acc, long n, float p, int seed, void* stream) {
  RV_REQUIRE(n % 8 == 0, "rv_dropout: n%8");
  RV_REQUIRE(p >= 0.f && p < 1.f, "rv_dropout: 0 <= p < 1");
  RV_REQUIRE(y != nullptr || acc != nullptr, "rv_dropout: need an output (y) or an accumulator (acc)");
  if (n == 0) return 0;
  const DropParams dp = drop_params(p, seed);                           // 16 random bits per element
  return launch<dropout_kernel>(0, dim3(grid_for(n / 8, 256)), dim3(256), stream, (const bf16_t*)x, (bf16_t*)y, (bf16_t*)acc, n / 8,
                                dp.thresh16, dp.inv_keep, dp.key);
}

int rv_resize_h_u8(const void* src, int H, int W, int y0, int rows, const int* bounds, const int* kk, int ksize, int out_w,
                   void* tmp, void* stream) {
  RV_REQUIRE(H > 0 && W > 0 && rows > 0 && y0 >= 0 && y0 + rows <= H && ksize > 0 && out_w > 0, "rv_resize_h_u8: bad sizes");
  const long n = (long)rows * out_w * 3;
  return launch<resize_h_u8_kernel>(0, dim3(grid_for(n, 256)), dim3(256), stream, (const uint8_t*)src, W, y0, rows, bounds, kk, ksize,
                                    out_w, (uint8_t*)tmp);
}
int rv_resize_v_norm_u8(const void* tmp, int rows, int out_w, const int* bounds, const int* kk, int ksize, int out_h,
                        const float* table, float* out, void* stream) {
  RV_REQUIRE(rows > 0 && out_w > 0 && out_h > 0 && ksize > 0, "rv_resize_v_norm_u8: bad sizes");
  const long n = 3L * out_h * out_w;
  return launch<resize_v_norm_u8_kernel>(0, dim3(grid_for(n, 256)), dim3(256), stream, (const uint8_t*)tmp, out_w, bounds, kk, ksize,
                                         out_h, table, out);
}

int rv_transpose(const void* in, long ld_in, void* out, long ldo, int R, int C, void* stream) {
  RV_REQUIRE(C % 8 == 0 && ld_in % 8 == 0 && ldo % 8 == 0, "rv_transpose: C, ld_in, ldo must be multiples of 8");
  RV_REQUIRE(ldo >= ((R + 63) / 64) * 64, "rv_transpose: ldo must be >= roundup(R,64)");
  if (R == 0 || C == 0) return 0;
  return launch<transpose_kernel>(0, dim3((C + 63) / 64, (R + 63) / 64), dim3(256), stream, (const bf16_t*)in, ld_in, (bf16_t*)out, ldo,
                                  R, C);
}

int rv_splice_fwd(const int* src, const void* embed, const void* feats, void* out, long n_rows, int d, void* stream) {
  RV_REQUIRE(d % 8 == 0, "rv_splice_fwd: d%8");
  if (n_rows == 0) return 0;
  return launch<splice_fwd_kernel>(0, dim3(grid_for(n_rows * (d / 8), 256, 16384)), dim3(256), stream, src, (const bf16_t*)embed,
                                   (const bf16_t*)feats, (bf16_t*)out, n_rows, d);
}

int rv_embed_bwd(const int* uniq_ids, const int* seg_off, const int* pos_sorted, int n_uniq, const void* dx, void* dW,
                 int d, void* stream) {
  RV_REQUIRE(d % 8 == 0, "rv_embed_bwd: d%8");
  if (n_uniq == 0) return 0;
  return launch<embed_bwd_kernel>(0, dim3(n_uniq), dim3(256), stream, uniq_ids, seg_off, pos_sorted, (const bf16_t*)dx, (bf16_t*)dW, d);
}

int rv_feat_grad(const int* src_a, const int* src_b, const void* dx, void* dfeat, long n_rows, int d, void* stream) {
  RV_REQUIRE(d % 8 == 0, "rv_feat_grad: d%8");
  if (n_rows == 0) return 0;
  return launch<feat_grad_kernel>(0, dim3(grid_for(n_rows * (d / 8), 256, 16384)), dim3(256), stream, src_a, src_b, (const bf16_t*)dx,
                                  (bf16_t*)dfeat, n_rows, d);
}

int rv_gather_rows(const void* in, long ld_in, const int* idx, void* out, long ld_out, long n_rows, int d, int scatter,
                   void* stream) {
  RV_REQUIRE(d % 8 == 0 && ld_in % 8 == 0 && ld_out % 8 == 0, "rv_gather_rows: alignment");
  if (n_rows == 0) return 0;
  return launch<gather_rows_kernel>(0, dim3(grid_for(n_rows * (d / 8), 256, 16384)), dim3(256), stream, (const bf16_t*)in, ld_in, idx,
                                    (bf16_t*)out, ld_out, n_rows, d, scatter);
}

int rv_colsum(const void* dy, long ld, void* db, int M, int N, void* stream) {
  if (N == 0) return 0;
  return launch<colsum_kernel>(0, dim3((N + 63) / 64), dim3(1024), stream, (const bf16_t*)dy, ld, (bf16_t*)db, M, N);
}

int rv_im2col_patches(const float* pixels, void* out, int B, int image_size, int patch, int Kp, void* stream) {
  RV_REQUIRE(image_size % patch == 0 && Kp >= 3 * patch * patch, "rv_im2col_patches: bad geometry");
  const int g = image_size / patch;
  const long total = (long)B * g * g * Kp;
  if (total == 0) return 0;
  return launch<im2col_kernel>(0, dim3(grid_for(total, 256, 16384)), dim3(256), stream, pixels, (bf16_t*)out, B, image_size, patch, Kp);
}

int rv_clip_assemble(const void* patch, const void* cls, const void* pos, void* x, int B, int P, int d, void* stream) {
  RV_REQUIRE(d % 8 == 0, "rv_clip_assemble: d%8");
  if (B == 0) return 0;
  return launch<clip_assemble_kernel>(0, dim3(grid_for((long)B * (P + 1) * (d / 8), 256)), dim3(256), stream, (const bf16_t*)patch,
                                      (const bf16_t*)cls, (const bf16_t*)pos, (bf16_t*)x, B, P, d);
}

int rv_sumsq_nblocks(void) { return 1024; }

int rv_grad_norm(const void* g, long n, float* partial, float max_norm, float pre_scale, float* out2, void* stream) {
  RV_REQUIRE(n % 8 == 0, "rv_grad_norm: n%8");
  if (const int rc = launch_sumsq(g, n, partial, stream)) return rc;
  return launch<gradnorm_finish_kernel>(0, dim3(1), dim3(256), stream, partial, 1024, max_norm, pre_scale, out2);
}

int rv_grad_sumsq(const void* g, long n, float* partial, float* out1, int accumulate, void* stream) {
  RV_REQUIRE(n % 8 == 0, "rv_grad_sumsq: n%8");
  if (const int rc = launch_sumsq(g, n, partial, stream)) return rc;
  return launch<sumsq_finish_kernel>(0, dim3(1), dim3(256), stream, partial, 1024, out1, accumulate);
}

int rv_clip_from_sumsq(const float* sumsq, float max_norm, float pre_scale, float* out2, void* stream) {
  return launch<clip_from_sumsq_kernel>(0, dim3(1), dim3(1), stream, sumsq, max_norm, pre_scale, out2);
}

int rv_grad_accum(float* acc, void* g, long n, int mode, float scale, void* stream) {
  RV_REQUIRE(n % 8 == 0 && mode >= 0 && mode <= 2, "rv_grad_accum: n % 8 == 0, mode in 0..2");
  if (n == 0) return 0;
  return launch<grad_accum_kernel>(0, dim3(grid_for(n / 8, 256, 8192)), dim3(256), stream, acc, (bf16_t*)g, n / 8, mode, scale);
}

int rv_adamw_step(void* p, float* master, float* m, float* v, const void* g, long n, float lr, float beta1, float beta2,
                  float eps, float wd, int step, const float* clip, void* stream) {
  RV_REQUIRE(n % 8 == 0, "rv_adamw_step: n%8");
  if (n == 0) return 0;
  const float bc1 = 1.f - powf(beta1, (float)step);
  const float bc2 = 1.f - powf(beta2, (float)step);
  return launch<adamw_kernel>(0, dim3(grid_for(n / 8, 256, 8192)), dim3(256), stream, (bf16_t*)p, master, m, v, (const bf16_t*)g, n / 8, lr,
                              beta1, beta2, eps, wd, bc1, sqrtf(bc2), clip);
}

int rv_logp_finish(const float* pmax, const float* psum, const float* tgt_logit, int nblk, int M, float* lse,
                   float* logp, void* stream) {
  if (M == 0) return 0;
  return launch<logp_finish_kernel>(0, dim3((M + 3) / 4), dim3(256), stream, pmax, psum, tgt_logit, nblk, M, lse, logp);
}

int rv_logp_finish_unpack(const float* pmax, const float* psum, const float* tgt_logit, int nblk, int M, const int* dst_a,
                          const int* dst_b, const int* dst_c, float* per_token, long n_per_token, float* compact, int n_compact,
                          void* stream) {
  if (M == 0) return 0;
  RV_REQUIRE(nblk > 0 && M > 0 && n_per_token >= 0 && n_compact >= 0, "rv_logp_finish_unpack: nblk, M > 0; sizes >= 0");
  RV_REQUIRE(dst_a && dst_b && dst_c, "rv_logp_finish_unpack: the three destination tables are required (-1 = no slot)");
  RV_REQUIRE((per_token || n_per_token == 0) && (compact || n_compact == 0), "rv_logp_finish_unpack: NULL output with a non-zero size");
  return launch<logp_finish_unpack_kernel>(0, dim3((M + 3) / 4), dim3(256), stream, pmax, psum, tgt_logit, nblk, M, dst_a, dst_b, dst_c,
                                           per_token, n_per_token, compact, n_compact);
}

int rv_next_token_scores(const float* logits, long ldl, int M, int V_valid, const int* seen_off, const int* seen_ids,
                         float penalty, const int* want_ids, int K, float* probs, float* logp, int* argmax, float* lse,
                         void* stream) {
  if (M == 0) return 0;
  RV_REQUIRE(M > 0 && V_valid > 0 && ldl >= V_valid && K >= 0, "rv_next_token_scores: M, V_valid > 0, ldl >= V_valid, K >= 0");
  RV_REQUIRE(logits && argmax && lse && (K == 0 || (want_ids && probs && logp)), "rv_next_token_scores: NULL buffer");
  RV_REQUIRE(penalty > 0.f, "rv_next_token_scores: the repetition penalty must be positive (1 = off)");
  RV_REQUIRE(seen_off == nullptr || seen_ids != nullptr, "rv_next_token_scores: seen_off without seen_ids");
  const bool pen = seen_off != nullptr && penalty != 1.0f;
  const size_t lds = pen ? (size_t)((V_valid + 31) / 32) * 4 : 0;
  RV_REQUIRE(lds <= 60000, "rv_next_token_scores: the seen-id bitmap (V_valid / 8 bytes) must fit in LDS");
  return launch<next_token_scores_kernel>((int)lds, dim3(M), dim3(256), stream, logits, ldl, V_valid, seen_off, seen_ids, penalty, want_ids,
                                          K, probs, logp, argmax, lse);
}

int rv_seq_sum(const float* logp, const float* weight, const int* seq_off, int n_seq, float* out_sum, float* out_cnt,
               void* stream) {
  if (n_seq == 0) return 0;
  return launch<seq_sum_kernel>(0, dim3(n_seq), dim3(256), stream, logp, weight, seq_off, out_sum, out_cnt);
}

int rv_dpo_loss(const float* seq_sum, const float* seq_cnt, const float* ref_win, const float* ref_rej, int B,
                float beta, int use_average, float sft_weight, float dpo_weight, float* per_pair, float* scalars,
                float* coef, void* stream) {
  RV_REQUIRE(B > 0, "rv_dpo_loss: B must be > 0");
  return launch<dpo_loss_kernel>(0, dim3(1), dim3(256), stream, seq_sum, seq_cnt, ref_win, ref_rej, B, beta, use_average, sft_weight,
                                 dpo_weight, per_pair, scalars, coef);
}

int rv_row_coef(const float* coef, const int* seq_of_row, const float* weight, float* out, int n, void* stream) {
  if (n == 0) return 0;
  return launch<row_coef_kernel>(0, dim3((n + 255) / 256), dim3(256), stream, coef, seq_of_row, weight, out, n);
}

int rv_attn_delta(const void* dO, long lddo, const void* O, long ldo, float* delta, int S, int L, int H, int hd,
                  void* stream) {
  RV_REQUIRE(hd % 2 == 0, "rv_attn_delta: hd even");
  const long total = (long)S * L * H;
  if (total == 0) return 0;
  return launch<attn_delta_kernel>(0, dim3(grid_for(total, 4, 16384)), dim3(256), stream, (const bf16_t*)dO, lddo, (const bf16_t*)O, ldo,
                                   delta, S, L, H, hd);
}

int rv_cast_f32_to_bf16(const float* in, void* out, long n, void* stream) {
  return launch_flat<cast_f32_bf16_kernel>(n, 8192, stream, in, (bf16_t*)out);
}
int rv_cast_bf16_to_f32(const void* in, float* out, long n, void* stream) {
  return launch_flat<cast_bf16_f32_kernel>(n, 8192, stream, (const bf16_t*)in, out);
}

int rv_reduce_copy_persistent(const void* a, const void* b, void* dst, long n, int n_wg, void* stream) {
  RV_REQUIRE(n % 8 == 0, "rv_reduce_copy_persistent: n must be a multiple of 8 bf16 elements");
  RV_REQUIRE(n_wg >= 1 && n_wg <= 256, "rv_reduce_copy_persistent: 1 <= n_wg <= 256");
  if (n == 0) return 0;
  return launch<reduce_copy_persistent_kernel>(0, dim3(n_wg), dim3(256), stream, (const u32x4_t*)a, (const u32x4_t*)b, (u32x4_t*)dst, n / 8);
}

}  // extern "C"
