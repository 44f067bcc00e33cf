// The sampler for vocabularies that do not fit rv_sample_token's registers (Llama-3: 128256 ids): rv_sample_token's
// distribution and draw with the row STREAMED from L2 / MALL, where the LM head has just written it, instead of held in
// registers.  Contracts: include/rlaifv_hip.h.
//
// One workgroup of 16 waves per row.  Wave w owns the contiguous ids [w SEG, (w + 1) SEG), SEG = ceil(V / 16) rounded up to a
// multiple of 256, and walks them in tiles of 256 ids: lane l holds ids tile + 4 l .. 4 l + 3 (one 16-byte load per lane, 1 KB
// per wave).  Vocabulary order is therefore (wave, tile, lane, element) and every reduction is lane-accumulate over the tiles,
// wave butterfly, then the 16 wave results in wave order: fixed, and a function of the row alone.
//
// Passes over the row: (1) max / arg-max, (2) Z = sum exp, and when sampling (3) top-p candidates, (4) the kept mass per
// wave, (5) the draw.  Pass 3 replaces rv_sample_token's 31 bisection passes over the row: a token of probability
// p <= thr = (1 - top_p) Z / (2 V) is dropped whatever the threshold turns out to be (V of them weigh at most half the mass
// that may be dropped), so only the tokens above thr - a handful on a peaked row - are written out, in vocabulary order, and
// the bisection runs over that list plus the summed mass M0 of the rest.  The first SW_CAP candidates of a wave stay in LDS,
// later ones go to the wave's SEG floats of the caller's workspace (a flat row: every token is a candidate).
//
// rv_sample_token_wide_topk (the TOPK variant of the kernel; 0 < top_k < V while sampling) finds tau_k, the top_k-th largest
// score, by a radix select on score_key: three histograms of 11 + 11 + 10 key bits in LDS (integer atomics; the candidate lists'
// storage, not yet in use), the first filled during pass 1, the other two in a pass of their own over the ids that match the
// digits chosen so far.  From then on a score below tau_k reads as -inf, so Z, the candidates (at most top_k + ties of them), the
// kept mass and the draw run over the survivors with the code and the order of the plain variant.
#include <math.h>

#include "common.hpp"
#include "host.hpp"
#include "rlaifv_hip.h"

#define SW_THREADS 1024
#define SW_WAVES 16
#define SW_TILE 256
#define SW_CAP 512
#define SW_MAXV 262144
#define SW_NONE 0x7fffffff

static inline int sw_seg(int V) { return ((V + SW_WAVES - 1) / SW_WAVES + SW_TILE - 1) / SW_TILE * SW_TILE; }

#define SW_BINS 2048

struct SwRow {
  const float* row;
  const uint32_t* bits;      // the seen ids of the row as a bit set, or nullptr
  int V, vec;
  float penalty, tdiv;
  float tau_k;               // TOPK: scores below it are dropped (-inf until the select is done)
};

// repetition penalty, then temperature: the same two operations wherever a logit is turned into a score
__device__ __forceinline__ float sw_value(const SwRow& r, int i, float l) {
  if (r.bits && ((r.bits[i >> 5] >> (i & 31)) & 1u)) l = l > 0.f ? l / r.penalty : l * r.penalty;
  return l / r.tdiv;
}

// the scores of ids i0 .. i0 + 3 (i0 a multiple of 4); -inf behind the row's end, which is never read
template <bool TOPK>
__device__ __forceinline__ void sw_load(const SwRow& r, int i0, float* x) {
  if (r.vec && i0 + 3 < r.V) {
    const float4 v4 = *(const float4*)(r.row + i0);
    x[0] = v4.x, x[1] = v4.y, x[2] = v4.z, x[3] = v4.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = i0 + e < r.V ? r.row[i0 + e] : -INFINITY;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) x[e] = i0 + e < r.V ? sw_value(r, i0 + e, x[e]) : -INFINITY;
  if constexpr (TOPK) {
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = x[e] < r.tau_k ? -INFINITY : x[e];
  }
}

// SW_DEPTH tiles of a wave in flight: the passes that cannot be unrolled as a whole (ballots, scans: one tile after the other) fetch
// the scores of tiles t .. t + SW_DEPTH - 1 first; a tile behind the wave's last one (nt, wave-uniform) is all -inf
#define SW_DEPTH 4
template <bool TOPK>
__device__ __forceinline__ void sw_load_group(const SwRow& r, int l0, int t, int nt, float (*x)[4]) {
#pragma unroll
  for (int k = 0; k < SW_DEPTH; ++k) {
    if (t + k < nt) {
      sw_load<TOPK>(r, l0 + (t + k) * SW_TILE, x[k]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) x[k][e] = -INFINITY;
    }
  }
}

__device__ __forceinline__ float sw_prob(float x, float x_top) { return x != -INFINITY ? expf(x - x_top) : 0.f; }

__device__ __forceinline__ int sw_block_min(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = red[0];
  for (int i = 1; i < SW_WAVES; ++i) r = min(r, red[i]);
  return r;
}

// one count per id with `on` into hist[d]: a plain LDS integer add per lane.  Most scores of a row share their leading key bits, so
// many lanes add to one address; counting such lanes once per wave (ballot + popcount, one add by the first of them) was measured
// and is SLOWER - 208 against 193 us per call at M = 8, V = 128256 - the LDS takes same-address adds of a wave well.
__device__ __forceinline__ void sw_hist_add(int* hist, bool on, int d) {
  if (on) atomicAdd(&hist[d], 1);
}

// The highest bin b of hist[SW_BINS] whose count together with the bins above it reaches k; k becomes what is left to find inside
// that bin.  Thread t looks at bins 2047 - 2 t and 2046 - 2 t: suffix counts by wave scan and the 16 wave totals.  The caller
// guarantees 1 <= k <= the sum of the histogram, so exactly one thread finds its bin.  Ends behind a barrier: hist may be cleared.
__device__ __forceinline__ int sw_pick_bin(const int* hist, int& k, int* redi, int* sel) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __syncthreads();                                                // the histogram is complete
  const int b0 = SW_BINS - 1 - 2 * tid, h0 = hist[b0], h1 = hist[b0 - 1];
  int inc = h0 + h1;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int n = __shfl_up(inc, o, 64);
    if (lane >= o) inc += n;
  }
  if (lane == 63) redi[wave] = inc;
  __syncthreads();
  int above = inc - (h0 + h1);
  for (int w = 0; w < wave; ++w) above += redi[w];
  if (above < k && k <= above + h0) sel[0] = b0, sel[1] = k - above;
  else if (above + h0 < k && k <= above + h0 + h1) sel[0] = b0 - 1, sel[1] = k - above - h0;
  __syncthreads();
  k = sel[1];
  return sel[0];
}

// TOPK = false is rv_sample_token_wide's kernel as it was (top_k unread)
template <bool TOPK>
__global__ __launch_bounds__(SW_THREADS) void sample_token_wide_kernel(const float* __restrict__ logits, long ldl, int V,
                                                                       const int* __restrict__ seen_off,
                                                                       const int* __restrict__ seen_ids, float penalty,
                                                                       float temperature, float top_p,
                                                                       const float* __restrict__ u, int vec, int seg,
                                                                       float* __restrict__ ws, int* __restrict__ token,
                                                                       float* __restrict__ logp, int top_k) {
  extern __shared__ uint32_t sw_bits[];            // [ceil(V / 32)] when the penalty is on
  __shared__ float cand[SW_WAVES][SW_CAP];
  __shared__ float red[SW_WAVES];
  __shared__ int redi[SW_WAVES];
  __shared__ float red_mx[SW_WAVES];
  __shared__ int red_ix[SW_WAVES];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool pen = seen_off != nullptr && penalty != 1.0f;
  if (pen) {
    const int nw = (V + 31) >> 5;
    for (int i = tid; i < nw; i += SW_THREADS) sw_bits[i] = 0u;
    __syncthreads();
    for (int i = seen_off[m] + tid; i < seen_off[m + 1]; i += SW_THREADS) {
      const int id = seen_ids[i];
      if (id >= 0 && id < V) atomicOr(&sw_bits[id >> 5], 1u << (id & 31));
    }
    __syncthreads();
  }
  const bool greedy = temperature == 0.f;
  SwRow r;
  r.row = logits + (long)m * ldl, r.bits = pen ? sw_bits : nullptr, r.V = V, r.vec = vec;
  r.penalty = penalty, r.tdiv = greedy ? 1.f : temperature, r.tau_k = -INFINITY;
  const int w0 = min(wave * seg, V), w1 = min(w0 + seg, V);       // the wave's ids
  const int nt = (w1 - w0 + SW_TILE - 1) / SW_TILE;
  const int l0 = w0 + 4 * lane;                                   // the lane's first id; w0 is a multiple of 256 or V

  int* hist = (int*)&cand[0][0];                                  // TOPK: SW_BINS counts, before the candidate lists are built
  int* sel = hist + SW_BINS;                                      //       and behind them the chosen bin and what is left of k
  if constexpr (TOPK) {
    for (int i = tid; i < SW_BINS; i += SW_THREADS) hist[i] = 0;
    __syncthreads();
  }
  // ---- pass 1: the maximum and its lowest index (TOPK: and the histogram of the scores' leading 11 key bits)
  float mx = -INFINITY;
  int ix = SW_NONE;
  if constexpr (!TOPK) {
#pragma unroll 4
    for (int t = 0; t < nt; ++t) {
      float x[4];
      sw_load<TOPK>(r, l0 + t * SW_TILE, x);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (x[e] > mx) mx = x[e], ix = l0 + t * SW_TILE + e;     // indices grow inside a lane: the first of equal maxima stays
    }
  } else {
    for (int t = 0; t < nt; t += SW_DEPTH) {
      float xs[SW_DEPTH][4];
      sw_load_group<TOPK>(r, l0, t, nt, xs);
#pragma unroll
      for (int g = 0; g < SW_DEPTH; ++g) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = l0 + (t + g) * SW_TILE + e;
          const bool in = t + g < nt && i < V;
          if (in && xs[g][e] > mx) mx = xs[g][e], ix = i;
          sw_hist_add(hist, in, (int)(score_key(xs[g][e]) >> 21));
        }
      }
    }
  }
  if constexpr (TOPK) {
    // ---- TopKLogitsWarper without the sort: tau_k = the largest score with at least top_k scores >= it; everything tied with
    // it stays.  The key's digits from the top: 11 bits (counted above), 11 bits, 10 bits.
    int k = top_k;
    uint32_t prefix = (uint32_t)sw_pick_bin(hist, k, redi, sel);
#pragma unroll 1
    for (int round = 0; round < 2; ++round) {
      const int shift = round == 0 ? 10 : 0, up = round == 0 ? 21 : 10, mask = round == 0 ? 2047 : 1023;
      for (int i = tid; i < SW_BINS; i += SW_THREADS) hist[i] = 0;
      __syncthreads();
      for (int t = 0; t < nt; t += SW_DEPTH) {
        float xs[SW_DEPTH][4];
        sw_load_group<TOPK>(r, l0, t, nt, xs);
#pragma unroll
        for (int g = 0; g < SW_DEPTH; ++g) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const uint32_t key = score_key(xs[g][e]);
            const bool in = t + g < nt && l0 + (t + g) * SW_TILE + e < V;
            sw_hist_add(hist, in && (key >> up) == prefix, (int)((key >> shift) & mask));
          }
        }
      }
      prefix = (prefix << (up - shift)) | (uint32_t)sw_pick_bin(hist, k, redi, sel);
    }
    r.tau_k = score_of_key(prefix);
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
  for (int w = 1; w < SW_WAVES; ++w)
    if (red_mx[w] > mx || (red_mx[w] == mx && red_ix[w] < ix)) mx = red_mx[w], ix = red_ix[w];
  if (ix == SW_NONE) ix = 0;                                      // a row without a finite maximum: stay inside the row
  const float x_top = mx;

  // ---- pass 2: Z
  float loc = 0.f;
#pragma unroll 4
  for (int t = 0; t < nt; ++t) {
    float x[4];
    sw_load<TOPK>(r, l0 + t * SW_TILE, x);
#pragma unroll
    for (int e = 0; e < 4; ++e) loc += sw_prob(x[e], x_top);
  }
  const float Z = block_sum(loc, red);
  if (greedy) {
    if (tid == 0) {
      token[m] = ix;
      logp[m] = (sw_value(r, ix, r.row[ix]) - x_top) - logf(Z);
    }
    return;
  }
  float wbase = 0.f;                                              // kept mass of the waves before this one, in wave order
  for (int w = 0; w < wave; ++w) wbase += red[w];
  float Zk = Z, tau = 0.f;
  if (top_p < 1.f) {
    // ---- pass 3: the candidates, in vocabulary order per wave, and the mass of the rest
    const float c = (1.f - top_p) * Z;
    const float thr = 0.5f * c / (float)V;
    float* spill = ws + ((long)m * SW_WAVES + wave) * seg;
    float m0 = 0.f;
    int cnt = 0;
    for (int t = 0; t < nt; t += SW_DEPTH) {
      float xs[SW_DEPTH][4];
      sw_load_group<TOPK>(r, l0, t, nt, xs);
#pragma unroll
      for (int k = 0; k < SW_DEPTH; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = sw_prob(xs[k][e], x_top);
          const bool is = p > thr;
          m0 += is ? 0.f : p;
          const unsigned long long mask = __ballot(is);
          if (mask) {
            if (is) {
              const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
              if (pos < SW_CAP) cand[wave][pos] = p; else spill[pos - SW_CAP] = p;
            }
            cnt += __popcll(mask);
          }
        }
      }
    }
    __threadfence_block();                                        // the spilled candidates are read back by other lanes
    const float M0 = block_sum(m0, red);
    // TopPLogitsWarper without the sort, as rv_sample_token: a token of probability v is dropped iff the mass of all tokens
    // <= v is <= 1 - top_p; bisect the bit pattern of v for the smallest kept value.  Every v <= thr has mass <= M0 <= c.
    uint32_t lo = 0u, hi = __float_as_uint(1.f);
    while (hi - lo > 1u) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      const float v = __uint_as_float(mid);
      float sacc = 0.f;
      for (int j = lane; j < cnt; j += 64) {
        const float p = j < SW_CAP ? cand[wave][j] : spill[j - SW_CAP];
        sacc += p <= v ? p : 0.f;
      }
      if (M0 + block_sum(sacc, red) > c) hi = mid; else lo = mid;
    }
    tau = __uint_as_float(hi);
    // ---- pass 4: the kept mass per wave (every kept token is a candidate: tau > thr)
    loc = 0.f;
    for (int j = lane; j < cnt; j += 64) {
      const float p = j < SW_CAP ? cand[wave][j] : spill[j - SW_CAP];
      loc += p >= tau ? p : 0.f;
    }
    Zk = block_sum(loc, red);
    wbase = 0.f;
    for (int w = 0; w < wave; ++w) wbase += red[w];
  }

  // ---- pass 5: the draw - running sum in vocabulary order from the wave's base
  const float target = u[m] * Zk;
  float run = wbase;
  int found = SW_NONE, last = -1;
  for (int t = 0; t < nt; t += SW_DEPTH) {
    float xs[SW_DEPTH][4];
    sw_load_group<TOPK>(r, l0, t, nt, xs);
#pragma unroll
    for (int k = 0; k < SW_DEPTH; ++k) {
      float p[4], s = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        p[e] = sw_prob(xs[k][e], x_top);
        p[e] = (p[e] >= tau && p[e] > 0.f) ? p[e] : 0.f;
        s += p[e];
      }
      if (__ballot(s > 0.f) != 0ull) {                            // a tile without a kept token is skipped (wave-uniform)
        float inc = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const float n = __shfl_up(inc, o, 64);
          if (lane >= o) inc += n;
        }
        float rl = run + (inc - s);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (p[e] > 0.f) {
            rl += p[e];
            last = l0 + (t + k) * SW_TILE + e;
            if (rl > target && found == SW_NONE) found = last;
          }
        }
        run += __shfl(inc, 63, 64);
      }
    }
  }
  found = sw_block_min(found, redi);
  last = -sw_block_min(-last, redi);
  if (tid == 0) {
    const int tok = max(found != SW_NONE ? found : last, 0);      // u Zk rounded past the total: the last kept token
    token[m] = tok;
    logp[m] = (sw_value(r, tok, r.row[tok]) - x_top) - logf(Zk);
  }
}

extern "C" long rv_sample_token_wide_workspace_floats(int M, int V_valid) {
  if (M < 1 || V_valid < 1 || V_valid > SW_MAXV) return 0;
  return (long)M * SW_WAVES * sw_seg(V_valid);
}

// top_k off (0, >= V_valid) or greedy: rv_sample_token_wide's kernel, whichever entry point asks
static int sample_token_wide_launch(const float* logits, long ldl, int M, int V_valid, const int* seen_off, const int* seen_ids,
                                    float penalty, float temperature, float top_p, int top_k, const float* u, int* token,
                                    float* logp, float* workspace, void* stream) {
  const bool pen = seen_off != nullptr && penalty != 1.0f;
  const int lds = pen ? (V_valid + 31) / 32 * 4 : 0;
  const int vec = (((uintptr_t)logits & 15) == 0 && ldl % 4 == 0) ? 1 : 0;
  if (top_k > 0 && top_k < V_valid && temperature != 0.f)
    return launch<sample_token_wide_kernel<true>>(lds, dim3(M), dim3(SW_THREADS), stream, logits, ldl, V_valid, seen_off, seen_ids,
                                                  penalty, temperature, top_p, u, vec, sw_seg(V_valid), workspace, token, logp, top_k);
  return launch<sample_token_wide_kernel<false>>(lds, dim3(M), dim3(SW_THREADS), stream, logits, ldl, V_valid, seen_off, seen_ids,
                                                 penalty, temperature, top_p, u, vec, sw_seg(V_valid), workspace, token, logp, top_k);
}

extern "C" int rv_sample_token_wide(const float* logits, long ldl, int M, int V_valid, const int* seen_off, const int* seen_ids,
                                    float penalty, float temperature, float top_p, const float* u, int* token, float* logp,
                                    float* workspace, long workspace_floats, void* stream) {
  RV_REQUIRE(M > 0, "rv_sample_token_wide: M must be >= 1");
  RV_REQUIRE(V_valid >= 1 && V_valid <= SW_MAXV, "rv_sample_token_wide: 1 <= V_valid <= 262144");
  RV_REQUIRE(ldl >= V_valid, "rv_sample_token_wide: ldl >= V_valid");
  RV_REQUIRE(logits && token && logp && workspace, "rv_sample_token_wide: NULL buffer");
  RV_REQUIRE((((uintptr_t)logits | (uintptr_t)workspace | (uintptr_t)token | (uintptr_t)logp) & 3) == 0,
             "rv_sample_token_wide: buffers must be 4-byte aligned");
  RV_REQUIRE(temperature >= 0.f, "rv_sample_token_wide: temperature must be >= 0 (0 = greedy)");
  RV_REQUIRE(top_p > 0.f, "rv_sample_token_wide: top_p must be > 0 (>= 1 keeps every token)");
  RV_REQUIRE(penalty > 0.f, "rv_sample_token_wide: the repetition penalty must be positive (1 = off)");
  RV_REQUIRE(temperature == 0.f || u != nullptr, "rv_sample_token_wide: sampling needs the uniforms u[M]");
  RV_REQUIRE(seen_off == nullptr || seen_ids != nullptr, "rv_sample_token_wide: seen_off without seen_ids");
  RV_REQUIRE(workspace_floats >= rv_sample_token_wide_workspace_floats(M, V_valid),
             "rv_sample_token_wide: workspace smaller than rv_sample_token_wide_workspace_floats(M, V_valid)");
  return sample_token_wide_launch(logits, ldl, M, V_valid, seen_off, seen_ids, penalty, temperature, top_p, 0, u, token, logp,
                                  workspace, stream);
}

extern "C" int rv_sample_token_wide_topk(const float* logits, long ldl, int M, int V_valid, const int* seen_off,
                                         const int* seen_ids, float penalty, float temperature, float top_p, int top_k,
                                         const float* u, int* token, float* logp, float* workspace, long workspace_floats,
                                         void* stream) {
  RV_REQUIRE(M > 0, "rv_sample_token_wide_topk: M must be >= 1");
  RV_REQUIRE(V_valid >= 1 && V_valid <= SW_MAXV, "rv_sample_token_wide_topk: 1 <= V_valid <= 262144");
  RV_REQUIRE(ldl >= V_valid, "rv_sample_token_wide_topk: ldl >= V_valid");
  RV_REQUIRE(logits && token && logp && workspace, "rv_sample_token_wide_topk: NULL buffer");
  RV_REQUIRE((((uintptr_t)logits | (uintptr_t)workspace | (uintptr_t)token | (uintptr_t)logp) & 3) == 0,
             "rv_sample_token_wide_topk: buffers must be 4-byte aligned");
  RV_REQUIRE(temperature >= 0.f, "rv_sample_token_wide_topk: temperature must be >= 0 (0 = greedy)");
  RV_REQUIRE(top_p > 0.f, "rv_sample_token_wide_topk: top_p must be > 0 (>= 1 keeps every token)");
  RV_REQUIRE(top_k >= 0, "rv_sample_token_wide_topk: top_k must be >= 0 (0 or >= V_valid keeps every token)");
  RV_REQUIRE(penalty > 0.f, "rv_sample_token_wide_topk: the repetition penalty must be positive (1 = off)");
  RV_REQUIRE(temperature == 0.f || u != nullptr, "rv_sample_token_wide_topk: sampling needs the uniforms u[M]");
  RV_REQUIRE(seen_off == nullptr || seen_ids != nullptr, "rv_sample_token_wide_topk: seen_off without seen_ids");
  RV_REQUIRE(workspace_floats >= rv_sample_token_wide_workspace_floats(M, V_valid),
             "rv_sample_token_wide_topk: workspace smaller than rv_sample_token_wide_workspace_floats(M, V_valid)");
  return sample_token_wide_launch(logits, ldl, M, V_valid, seen_off, seen_ids, penalty, temperature, top_p, top_k, u, token, logp,
                                  workspace, stream);
}
