// Beam-search decoding (the evaluation stage: generate(do_sample=False, num_beams=K)): the two kernels a beam step adds behind
// the LM head - the per-group top-2K over log_softmax(logits) + beam score, and the device-side beam bookkeeping (running
// beams, finished hypotheses, stop rule, token history and cache-row table).  The attention that reads the row table is
// rv_attn_decode_indexed in decode.hip.  Contracts: include/rlaifv_hip.h.
#include <math.h>

#include "common.hpp"
#include "host.hpp"
#include "rlaifv_hip.h"

#define BT_THREADS 1024
#define BT_MAXK 8
#define BT_NONE 0x7fffffff
#define BT_DEAD (-1.0e9f)      // HF's score of beams 1..K-1 at step 0, and what it adds to a candidate that may not be chosen

// (value, index) order of every selection here: the larger value first, equal values by the lower index.  index == BT_NONE
// is "no element" and loses to everything.
__device__ __forceinline__ bool bt_better(float av, int ai, float bv, int bi) {
  if (ai == BT_NONE) return false;
  if (bi == BT_NONE) return true;
  return av > bv || (av == bv && ai < bi);
}
// an element still to be chosen after (wv, wi) was: strictly behind it in that order
__device__ __forceinline__ bool bt_after(float v, int i, float wv, int wi) { return v < wv || (v == wv && i > wi); }

// ------------------------------------------------------------------ per-row top-n of log_softmax(row) + score
// One workgroup of 1024 threads per row, the row in registers as in sample_token_kernel (thread t keeps ids [t IPT,
// (t + 1) IPT)).  n = 2K rounds of a block arg-max: every thread keeps the best of its not yet chosen elements, the round's
// winner is found by a wave butterfly and a pass over the 16 wave results in wave order, and only the thread that owned the
// winner looks through its registers again.  "Not yet chosen" is "strictly behind the last winner in the order", so no
// element is marked and a value may be anything finite.
// PEN (rv_beam_topk_penalty with a history and penalty != 1) puts HF's RepetitionPenaltyLogitsProcessor between the log-softmax
// and the score add: the row's history ids become an LDS bit set of ceil(V / 32) words, as in sample_token_kernel (a set: a
// duplicate id counts once), and a thread reads the one or two words that cover its ids - p[] is never indexed with an id.
// PEN = false is rv_beam_topk's kernel as it was, `pen` unread.
struct BeamPenalty {
  const int* hist;
  long ld_h;
  int n_hist;
  float penalty;
};

template <int IPT, bool PEN>
__global__ __launch_bounds__(BT_THREADS) void beam_topk_row_kernel(const float* __restrict__ logits, long ldl, int V,
                                                                   const float* __restrict__ score, int vec, int n,
                                                                   float* __restrict__ row_val, int* __restrict__ row_tok,
                                                                   float* __restrict__ lse, const BeamPenalty pen) {
  extern __shared__ uint32_t bt_bits[];            // [ceil(V / 32)] when PEN
  __shared__ float red[16];
  __shared__ float red_v[16];
  __shared__ int red_i[16];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* row = logits + (long)m * ldl;
  const int base = tid * IPT;
  if constexpr (PEN) {
    const int nw = (V + 31) >> 5;
    for (int i = tid; i < nw; i += BT_THREADS) bt_bits[i] = 0u;
    __syncthreads();
    const int* h = pen.hist + (long)m * pen.ld_h;
    for (int i = tid; i < pen.n_hist; i += BT_THREADS) {
      const int id = h[i];
      if (id >= 0 && id < V) atomicOr(&bt_bits[id >> 5], 1u << (id & 31));
    }
    __syncthreads();                                   // also stands before the first read of bt_bits below
  }
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
#pragma unroll
  for (int e = 0; e < IPT; ++e) mx = fmaxf(mx, p[e]);
  mx = wave_max(mx);
  if (lane == 0) red_v[wave] = mx;
  __syncthreads();
  mx = red_v[0];
  for (int w = 1; w < BT_THREADS / 64; ++w) mx = fmaxf(mx, red_v[w]);
  float loc = 0.f;
#pragma unroll
  for (int e = 0; e < IPT; ++e) loc += base + e < V ? expf(p[e] - mx) : 0.f;
  const float logz = logf(block_sum(loc, red));
  const float sc = score[m];
  if constexpr (PEN) {
    // HF's rule is l < 0 ? l * penalty : l / penalty.  A log-probability is never positive here: the row's maximum gives
    // x - mx = +0 and contributes expf(0) = 1 to Z, so log Z >= +0 and l <= +0; the division is met by l = +0 alone, where it
    // gives the product's +0 (a NaN stays a NaN either way).  So the product IS the rule, and the division's temporaries do not
    // push the 64-ids-per-thread instantiation (128 VGPRs at 1024 threads) into scratch.
    // ids [base + c, base + c + BT_CHUNK) lie in one word of the set (base is a multiple of IPT, BT_CHUNK divides 32); a word is
    // read only where its first id is valid, and an id >= V of a valid word has no bit (the fill checks id < V)
    constexpr int BT_CHUNK = IPT < 32 ? IPT : 32;
#pragma unroll
    for (int c = 0; c < IPT; c += BT_CHUNK) {
      const uint32_t w = base + c < V ? bt_bits[(base + c) >> 5] >> ((base + c) & 31) : 0u;
#pragma unroll
      for (int e = c; e < c + BT_CHUNK; ++e) {
        float l = (p[e] - mx) - logz;                  // log_softmax in fp32 ...
        if ((w >> (e - c)) & 1u) l = __fmul_rn(l, pen.penalty);     // ... HF's processor on it, never fused with the add ...
        p[e] = l + sc;                                 // ... then ONE add (HF's order)
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < IPT; ++e) p[e] = ((p[e] - mx) - logz) + sc;      // log_softmax in fp32, then ONE add (HF's order)
  }
  if (tid == 0) lse[m] = mx + logz;
  float bv = 0.f, wv = 0.f;
  int bi = BT_NONE, wi = -1;
#pragma unroll
  for (int e = 0; e < IPT; ++e)
    if (base + e < V && bt_better(p[e], base + e, bv, bi)) bv = p[e], bi = base + e;
  for (int r = 0; r < n; ++r) {
    float cv = bv;
    int ci = bi;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float v2 = __shfl_xor(cv, o, 64);
      const int i2 = __shfl_xor(ci, o, 64);
      if (bt_better(v2, i2, cv, ci)) cv = v2, ci = i2;
    }
    __syncthreads();                                   // the previous round's reads of red_v / red_i are over
    if (lane == 0) red_v[wave] = cv, red_i[wave] = ci;
    __syncthreads();
    wv = red_v[0], wi = red_i[0];
    for (int w = 1; w < BT_THREADS / 64; ++w)
      if (bt_better(red_v[w], red_i[w], wv, wi)) wv = red_v[w], wi = red_i[w];
    if (tid == 0) row_val[(long)m * n + r] = wv, row_tok[(long)m * n + r] = wi;
    if (bi == wi) {                                    // the owner: its next best behind the winner
      bv = 0.f, bi = BT_NONE;
#pragma unroll
      for (int e = 0; e < IPT; ++e)
        if (base + e < V && bt_after(p[e], base + e, wv, wi) && bt_better(p[e], base + e, bv, bi)) bv = p[e], bi = base + e;
    }
  }
}

// One wave per group: the n best of the K sorted row lists (K n <= 128 entries, two per lane), ordered by value, then by the
// flat index beam * V + token.
__global__ __launch_bounds__(64) void beam_topk_merge_kernel(const float* __restrict__ row_val, const int* __restrict__ row_tok,
                                                             int K, int V, int n, float* __restrict__ cand_val,
                                                             int* __restrict__ cand_parent, int* __restrict__ cand_tok) {
  const int g = blockIdx.x, lane = threadIdx.x, total = K * n;
  float v[2];
  int f[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int i = lane + 64 * s;
    v[s] = 0.f, f[s] = BT_NONE;
    if (i < total) {
      const int beam = i / n;
      v[s] = row_val[((long)g * K + beam) * n + (i - beam * n)];
      f[s] = beam * V + row_tok[((long)g * K + beam) * n + (i - beam * n)];
    }
  }
  float wv = 0.f;
  int wf = -1;
  for (int r = 0; r < n; ++r) {
    float cv = 0.f;
    int cf = BT_NONE;
#pragma unroll
    for (int s = 0; s < 2; ++s)
      if (f[s] != BT_NONE && (r == 0 || bt_after(v[s], f[s], wv, wf)) && bt_better(v[s], f[s], cv, cf)) cv = v[s], cf = f[s];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float v2 = __shfl_xor(cv, o, 64);
      const int f2 = __shfl_xor(cf, o, 64);
      if (bt_better(v2, f2, cv, cf)) cv = v2, cf = f2;
    }
    wv = cv, wf = cf;
    if (lane == 0) {
      cand_val[(long)g * n + r] = wv;
      cand_parent[(long)g * n + r] = wf / V;
      cand_tok[(long)g * n + r] = wf - (wf / V) * V;
    }
  }
}

extern "C" long rv_beam_topk_workspace_floats(int G, int K) {
  if (G < 1 || K < 1 || K > BT_MAXK) return 0;
  return (long)G * K * 2 * K * 2;                       // per row 2K values, then per row 2K tokens
}

// the checks and the two launches of rv_beam_topk and rv_beam_topk_penalty; pen.hist == nullptr = the plain kernel
static int beam_topk_run(const char* who, const float* logits, long ldl, const float* score, int G, int K, int V_valid,
                         const BeamPenalty pen, float* cand_val, int* cand_parent, int* cand_tok, float* lse, float* workspace,
                         long workspace_floats, void* stream) {
  RV_REQUIRE_AS(who, K >= 1 && K <= BT_MAXK, "1 <= K <= 8 beams");
  RV_REQUIRE_AS(who, G >= 1 && (long)G * K <= 65535, "G >= 1, G * K <= 65535 rows");
  RV_REQUIRE_AS(who, V_valid <= BT_THREADS * 64, "V_valid <= 65536 (the row is held in registers)");
  RV_REQUIRE_AS(who, V_valid >= 2 * K && ldl >= V_valid, "V_valid >= 2 K candidates per row, ldl >= V_valid");
  RV_REQUIRE_AS(who, logits && score && cand_val && cand_parent && cand_tok && lse && workspace, "NULL buffer");
  RV_REQUIRE_AS(who, (((uintptr_t)logits | (uintptr_t)score | (uintptr_t)cand_val | (uintptr_t)cand_parent | (uintptr_t)cand_tok |
                       (uintptr_t)lse | (uintptr_t)workspace) & 3) == 0, "buffers must be 4-byte aligned");
  RV_REQUIRE_AS(who, workspace_floats >= rv_beam_topk_workspace_floats(G, K),
                "workspace smaller than rv_beam_topk_workspace_floats(G, K)");
  const int M = G * K, n = 2 * K;
  float* row_val = workspace;
  int* row_tok = (int*)(workspace + (long)M * n);
  const int vec = (((uintptr_t)logits & 15) == 0 && ldl % 4 == 0) ? 1 : 0;
  const int lds = pen.hist ? ((V_valid + 31) >> 5) * 4 : 0;
#define BT_LAUNCH(IPT)                                                                                                          \
  (pen.hist ? launch<beam_topk_row_kernel<IPT, true>>(lds, dim3(M), dim3(BT_THREADS), stream, logits, ldl, V_valid, score, vec, n, \
                                                      row_val, row_tok, lse, pen)                                               \
            : launch<beam_topk_row_kernel<IPT, false>>(0, dim3(M), dim3(BT_THREADS), stream, logits, ldl, V_valid, score, vec, n, \
                                                       row_val, row_tok, lse, pen))
  int rc;
  if (V_valid <= BT_THREADS * 8) rc = BT_LAUNCH(8);
  else if (V_valid <= BT_THREADS * 32) rc = BT_LAUNCH(32);
  else rc = BT_LAUNCH(64);
#undef BT_LAUNCH
  if (rc) return rc;
  return launch<beam_topk_merge_kernel>(0, dim3(G), dim3(64), stream, (const float*)row_val, (const int*)row_tok, K, V_valid, n,
                                        cand_val, cand_parent, cand_tok);
}

extern "C" int rv_beam_topk(const float* logits, long ldl, const float* score, int G, int K, int V_valid, float* cand_val,
                            int* cand_parent, int* cand_tok, float* lse, float* workspace, long workspace_floats, void* stream) {
  return beam_topk_run("rv_beam_topk", logits, ldl, score, G, K, V_valid, BeamPenalty{nullptr, 0, 0, 1.f}, cand_val, cand_parent,
                       cand_tok, lse, workspace, workspace_floats, stream);
}

extern "C" int rv_beam_topk_penalty(const float* logits, long ldl, const float* score, int G, int K, int V_valid, const int* hist,
                                    long ld_h, int n_hist, float penalty, float* cand_val, int* cand_parent, int* cand_tok,
                                    float* lse, float* workspace, long workspace_floats, void* stream) {
  const char* who = "rv_beam_topk_penalty";
  RV_REQUIRE_AS(who, penalty > 0.f, "penalty must be > 0 (1 = off)");               // false for a NaN as well
  RV_REQUIRE_AS(who, n_hist >= 0 && n_hist <= ld_h, "0 <= n_hist <= ld_h (the row length of the history table)");
  RV_REQUIRE_AS(who, hist != nullptr || n_hist == 0 || penalty == 1.f, "hist is NULL with n_hist > 0 and penalty != 1");
  RV_REQUIRE_AS(who, ((uintptr_t)hist & 3) == 0, "hist must be 4-byte aligned");
  RV_REQUIRE_AS(who, G < 1 || K < 1 || ld_h <= 0x7fffffffL / ((long)G * K), "G * K * ld_h must fit int32");
  const bool on = hist != nullptr && n_hist > 0 && penalty != 1.f;                  // else: rv_beam_topk's kernel, its bits
  const BeamPenalty pen = on ? BeamPenalty{hist, ld_h, n_hist, penalty} : BeamPenalty{nullptr, 0, 0, 1.f};
  return beam_topk_run(who, logits, ldl, score, G, K, V_valid, pen, cand_val, cand_parent, cand_tok, lse, workspace,
                       workspace_floats, stream);
}

// ------------------------------------------------------------------ one beam step
// One wave per group.  Lane 0 restates GenerationMixin._beam_search's steps d - g on the group's 2K candidates (they are few:
// a serial pass), the wave then copies: the finished hypotheses' tokens, and the two per-beam tables from buffer A to buffer B.
struct BeamStepArgs {
  const float* cand_val;
  const int* cand_parent;
  const int* cand_tok;
  const int* force_parent;
  const int* force_token;
  const float* force_score;
  float* run_score;
  int* parent;
  int* token;
  const int* hist_a;
  int* hist_b;
  const int* rows_a;
  int* rows_b;
  int* hyp_tokens;
  int* hyp_len;
  float* hyp_score;
  int* n_hyp;
  int* done;
  long ld_t;
  int K, T, j, eos, last, own_base, M;
  float len_div;
};

__global__ __launch_bounds__(64) void beam_step_kernel(const BeamStepArgs a) {
  __shared__ int s_parent[BT_MAXK], s_token[BT_MAXK], s_job_slot[BT_MAXK], s_job_cand[BT_MAXK], s_njobs;
  __shared__ float rs[BT_MAXK];                          // the new running scores (LDS: lane 0 indexes them at run time)
  const int g = blockIdx.x, lane = threadIdx.x, K = a.K, n = 2 * K, j = a.j;
  const float* cv = a.cand_val + (long)g * n;
  const int* cp = a.cand_parent + (long)g * n;
  const int* ct = a.cand_tok + (long)g * n;
  if (lane == 0) {
    const bool forced = a.force_parent != nullptr;
    const bool frozen = forced || a.done[g] != 0;
    // e. the K running beams: the best candidates that hit no stopping criterion, in order; what is short of K (only when
    //    every candidate stops: the last step) is filled in candidate order at value - 1e9, as the reference's top-k does
    int nr = 0;
    bool all_hit = true;
    for (int c = 0; c < n; ++c) {
      const bool hit = a.last || ct[c] == a.eos;
      all_hit = all_hit && hit;
      if (!hit && nr < K) s_parent[nr] = min(max(cp[c], 0), K - 1), s_token[nr] = ct[c], rs[nr] = cv[c], ++nr;
    }
    for (int c = 0; c < n && nr < K; ++c)
      if (a.last || ct[c] == a.eos) s_parent[nr] = min(max(cp[c], 0), K - 1), s_token[nr] = ct[c], rs[nr] = cv[c] + BT_DEAD, ++nr;
    if (forced)
      for (int b = 0; b < K; ++b)
        s_parent[b] = min(max(a.force_parent[g * K + b], 0), K - 1), s_token[b] = a.force_token[g * K + b],
        rs[b] = a.force_score[g * K + b];
    // f. candidates of rank < K that stopped become finished hypotheses: the set keeps the K best length-normalised scores
    int njobs = 0;
    if (!frozen) {
      int nh = a.n_hyp[g];
      for (int c = 0; c < K; ++c) {
        if (!(a.last || ct[c] == a.eos)) continue;
        const float s = cv[c] / a.len_div;
        int slot = nh;
        if (nh == K) {                                  // full: the worst goes, if the new one is strictly better
          slot = 0;
          for (int h = 1; h < K; ++h)
            if (a.hyp_score[g * K + h] < a.hyp_score[g * K + slot]) slot = h;
          if (!(s > a.hyp_score[g * K + slot])) continue;
        } else {
          ++nh;
        }
        a.hyp_score[g * K + slot] = s;
        a.hyp_len[g * K + slot] = j + 1;
        s_job_slot[njobs] = slot, s_job_cand[njobs] = c, ++njobs;
      }
      a.n_hyp[g] = nh;
      // g. the stop rule (early_stopping=False): can the best running beam still beat the worst finished hypothesis?
      float worst = BT_DEAD;
      if (nh == K) {
        worst = a.hyp_score[g * K];
        for (int h = 1; h < K; ++h) worst = fminf(worst, a.hyp_score[g * K + h]);
      }
      const bool improvable = rs[0] / a.len_div > worst;
      a.done[g] = (all_hit || !improvable) ? 1 : 0;
    }
    s_njobs = njobs;
    for (int b = 0; b < K; ++b) {
      a.run_score[g * K + b] = rs[b];
      a.parent[g * K + b] = s_parent[b];
      a.token[g * K + b] = s_token[b];
    }
  }
  __syncthreads();
  for (int q = 0; q < s_njobs; ++q) {
    const int c = s_job_cand[q];
    int* dst = a.hyp_tokens + ((long)g * K + s_job_slot[q]) * a.T;
    const int* src = a.hist_a + ((long)g * K + min(max(cp[c], 0), K - 1)) * a.ld_t;    // a parent is clamped: never a row outside the group
    for (int t = lane; t < j; t += 64) dst[t] = src[t];
    if (lane == 0) dst[j] = ct[c];
  }
  for (int b = 0; b < K; ++b) {
    const long srow = ((long)g * K + s_parent[b]) * a.ld_t, drow = ((long)g * K + b) * a.ld_t;
    for (int t = lane; t < j; t += 64) {
      a.hist_b[drow + t] = a.hist_a[srow + t];
      a.rows_b[drow + t] = a.rows_a[srow + t];
    }
    if (lane == 0) {
      a.hist_b[drow + j] = s_token[b];
      a.rows_b[drow + j] = a.own_base + j * a.M + (g * K + b);       // step-major: the row this token's K | V will be written to
    }
  }
}

static bool bs_overlap(const void* p, const void* q, long bytes) {
  const uintptr_t x = (uintptr_t)p, y = (uintptr_t)q;
  return x < y ? y - x < (uintptr_t)bytes : x - y < (uintptr_t)bytes;
}

extern "C" int rv_beam_step(const float* cand_val, const int* cand_parent, const int* cand_tok, int G, int K, int T, int j,
                            int eos_token_id, float len_div, int last, int own_base, const int* force_parent,
                            const int* force_token, const float* force_score, float* run_score, int* parent, int* token,
                            const int* hist_a, int* hist_b, const int* rows_a, int* rows_b, long ld_t, int* hyp_tokens,
                            int* hyp_len, float* hyp_score, int* n_hyp, int* done, void* stream) {
  RV_REQUIRE(K >= 1 && K <= BT_MAXK, "rv_beam_step: 1 <= K <= 8 beams");
  RV_REQUIRE(G >= 1 && (long)G * K <= 65535, "rv_beam_step: G >= 1, G * K <= 65535 rows");
  RV_REQUIRE(T >= 1 && j >= 0 && j < T, "rv_beam_step: T >= 1, 0 <= j < T");
  RV_REQUIRE(ld_t >= T, "rv_beam_step: ld_t (the row length of the token history and the row table) must be >= T");
  RV_REQUIRE(last == 0 || last == 1, "rv_beam_step: last is 0 or 1");
  RV_REQUIRE(last == (j == T - 1 ? 1 : 0), "rv_beam_step: last must be set at step T - 1 and only there");
  RV_REQUIRE(len_div > 0.f, "rv_beam_step: len_div = (j + 1) ** length_penalty must be positive");
  RV_REQUIRE(own_base >= 0 && (long)own_base + (long)T * G * K <= 0x7fffffffL, "rv_beam_step: own_base + T * G * K must fit int32");
  RV_REQUIRE(cand_val && cand_parent && cand_tok && run_score && parent && token && hist_a && hist_b && rows_a && rows_b &&
                 hyp_tokens && hyp_len && hyp_score && n_hyp && done, "rv_beam_step: NULL buffer");
  RV_REQUIRE((force_parent == nullptr) == (force_token == nullptr) && (force_parent == nullptr) == (force_score == nullptr),
             "rv_beam_step: force_parent, force_token and force_score come together or not at all");
  RV_REQUIRE((((uintptr_t)cand_val | (uintptr_t)cand_parent | (uintptr_t)cand_tok | (uintptr_t)run_score | (uintptr_t)parent |
               (uintptr_t)token | (uintptr_t)hist_a | (uintptr_t)hist_b | (uintptr_t)rows_a | (uintptr_t)rows_b |
               (uintptr_t)hyp_tokens | (uintptr_t)hyp_len | (uintptr_t)hyp_score | (uintptr_t)n_hyp | (uintptr_t)done |
               (uintptr_t)force_parent | (uintptr_t)force_token | (uintptr_t)force_score) & 3) == 0,
             "rv_beam_step: buffers must be 4-byte aligned");
  const long tbytes = (long)G * K * ld_t * 4;
  RV_REQUIRE(!bs_overlap(hist_a, hist_b, tbytes) && !bs_overlap(rows_a, rows_b, tbytes),
             "rv_beam_step: buffer A and buffer B of a table must be distinct (an in-place gather is a race between beams)");
  BeamStepArgs a;
  a.cand_val = cand_val, a.cand_parent = cand_parent, a.cand_tok = cand_tok;
  a.force_parent = force_parent, a.force_token = force_token, a.force_score = force_score;
  a.run_score = run_score, a.parent = parent, a.token = token;
  a.hist_a = hist_a, a.hist_b = hist_b, a.rows_a = rows_a, a.rows_b = rows_b;
  a.hyp_tokens = hyp_tokens, a.hyp_len = hyp_len, a.hyp_score = hyp_score, a.n_hyp = n_hyp, a.done = done;
  a.ld_t = ld_t, a.K = K, a.T = T, a.j = j, a.eos = eos_token_id, a.last = last, a.own_base = own_base, a.M = G * K;
  a.len_div = len_div;
  return launch<beam_step_kernel>(0, dim3(G), dim3(64), stream, a);
}
