// Per-slot decode state of continuous batching (LlavaDPOModel.generate_continuous): the bookkeeping between the sampler and
// the next decode step when every row of the step is at a step of its own.  Two kernels: rv_decode_advance records each
// live slot's sampled token and emits what the next step's launches read (token, RoPE position, cache row, key spans,
// uniform); rv_decode_admit hands a list of slots to new sequences and advances them by their first token.  A finished or
// unused slot is parked on the first row of its own cache region.  Contracts: include/rlaifv_hip.h.
#include <stdint.h>

#include "host.hpp"
#include "rlaifv_hip.h"

#define DS_MAX_EOS 8
#define DS_MAX_ADMIT 64
#define DS_THREADS 64

struct DecodeStateArgs {
  const int* token;              // sampled tokens: [S] by slot (advance), [n] by list entry (admit)
  int *len, *budget, *done, *pre_off, *pre_len;
  const int* own_off;
  int *out_tokens, *seen_ids;
  const float* u_table;
  long ld_t;
  int S, T, n_eos;
  int eos[DS_MAX_EOS];
  int *tok_in, *pos, *dst, *pre_len_eff, *own_len;
  float* u_next;
};

struct DecodeAdmitList {
  int n;
  int slot[DS_MAX_ADMIT], pre_off[DS_MAX_ADMIT], pre_len[DS_MAX_ADMIT], budget[DS_MAX_ADMIT];
};

// One slot, one thread.  Every index into a table or a cache region is derived from values clamped here, so a corrupted
// state array parks the slot or misplaces a token inside the slot's own row, never outside it.
__device__ __forceinline__ void ds_advance_slot(const DecodeStateArgs& a, int s, int tok) {
  const int b = min(max(a.budget[s], 0), a.T);
  int l = a.len[s];
  int d = a.done[s];
  if (d == 0 && (l < 0 || l >= b)) {                     // a live slot without room: finished, nothing recorded
    d = 1;
    a.done[s] = 1;
  }
  if (d == 0) {
    const long at = (long)s * a.ld_t + l;
    a.out_tokens[at] = tok;
    a.seen_ids[at] = tok;
    l += 1;
    a.len[s] = l;
    bool stop = l >= b;
    for (int e = 0; e < a.n_eos; ++e) stop = stop || tok == a.eos[e];
    if (stop) {
      d = 1;
      a.done[s] = 1;
    }
  }
  const int own = a.own_off[s];
  if (d == 0) {                                          // 1 <= l < b <= T: column l of the tables and row l - 1 of the region exist
    const int pl = a.pre_len[s];
    a.tok_in[s] = tok;
    a.pos[s] = pl + l - 1;
    a.dst[s] = own + l - 1;
    a.pre_len_eff[s] = pl;
    a.own_len[s] = l;
    a.u_next[s] = a.u_table[(long)s * a.ld_t + l];
  } else {                                               // parked: writes and attends row 0 of its own region
    a.tok_in[s] = 0;
    a.pos[s] = 0;
    a.dst[s] = own;
    a.pre_len_eff[s] = 0;
    a.own_len[s] = 1;
    a.u_next[s] = 0.5f;
  }
}

__global__ void __launch_bounds__(DS_THREADS) decode_advance_kernel(DecodeStateArgs a) {
  const int s = blockIdx.x * DS_THREADS + threadIdx.x;
  if (s < a.S) ds_advance_slot(a, s, a.token[s]);
}

// One workgroup per admitted slot: its threads reset the slot's row of seen_ids, then thread 0 takes the slot over.
__global__ void __launch_bounds__(DS_THREADS) decode_admit_kernel(DecodeStateArgs a, DecodeAdmitList q) {
  const int i = blockIdx.x;
  const int s = q.slot[i];
  for (int t = threadIdx.x; t < a.T; t += DS_THREADS) a.seen_ids[(long)s * a.ld_t + t] = -1;
  __syncthreads();
  if (threadIdx.x == 0) {
    a.len[s] = 0;
    a.done[s] = 0;
    a.pre_off[s] = q.pre_off[i];
    a.pre_len[s] = q.pre_len[i];
    a.budget[s] = q.budget[i];
    ds_advance_slot(a, s, a.token[i]);
  }
}

static int ds_fill(const char* who, DecodeStateArgs& a, const int* token, int* len, int* budget, int* done, int* pre_off,
                   int* pre_len, const int* own_off, const int* eos_ids, int n_eos, int* out_tokens, int* seen_ids,
                   const float* u_table, long ld_t, int S, int T, int* tok_in, int* pos, int* dst, int* pre_len_eff, int* own_len,
                   float* u_next) {
  RV_REQUIRE_AS(who, S >= 1 && S <= 65535 * DS_THREADS, "S >= 1 slots");
  RV_REQUIRE_AS(who, T >= 1 && ld_t >= T, "T >= 1 columns, ld_t >= T");
  RV_REQUIRE_AS(who, (long)S * ld_t <= 0x7fffffffL, "S * ld_t must fit int32");
  RV_REQUIRE_AS(who, n_eos >= 0 && n_eos <= DS_MAX_EOS, "0 <= n_eos <= 8 EOS ids");
  RV_REQUIRE_AS(who, n_eos == 0 || eos_ids != nullptr, "NULL eos_ids with n_eos > 0");
  RV_REQUIRE_AS(who, out_tokens && seen_ids && u_table, "NULL table (out_tokens, seen_ids, u_table)");
  RV_REQUIRE_AS(who, token && len && budget && done && pre_off && pre_len && own_off, "NULL state array");
  RV_REQUIRE_AS(who, tok_in && pos && dst && pre_len_eff && own_len && u_next, "NULL output array");
  RV_REQUIRE_AS(who, (((uintptr_t)token | (uintptr_t)len | (uintptr_t)budget | (uintptr_t)done | (uintptr_t)pre_off |
                       (uintptr_t)pre_len | (uintptr_t)own_off | (uintptr_t)out_tokens | (uintptr_t)seen_ids | (uintptr_t)u_table |
                       (uintptr_t)tok_in | (uintptr_t)pos | (uintptr_t)dst | (uintptr_t)pre_len_eff | (uintptr_t)own_len |
                       (uintptr_t)u_next) & 3) == 0, "buffers must be 4-byte aligned");
  a.token = token, a.len = len, a.budget = budget, a.done = done, a.pre_off = pre_off, a.pre_len = pre_len, a.own_off = own_off;
  a.out_tokens = out_tokens, a.seen_ids = seen_ids, a.u_table = u_table, a.ld_t = ld_t, a.S = S, a.T = T, a.n_eos = n_eos;
  for (int e = 0; e < DS_MAX_EOS; ++e) a.eos[e] = e < n_eos ? eos_ids[e] : -1;
  a.tok_in = tok_in, a.pos = pos, a.dst = dst, a.pre_len_eff = pre_len_eff, a.own_len = own_len, a.u_next = u_next;
  return 0;
}

extern "C" int rv_decode_advance(const int* token, int* len, const int* budget, int* done, const int* pre_off, const int* pre_len,
                                 const int* own_off, const int* eos_ids, int n_eos, int* out_tokens, int* seen_ids,
                                 const float* u_table, long ld_t, int S, int T, int* tok_in, int* pos, int* dst, int* pre_len_eff,
                                 int* own_len, float* u_next, void* stream) {
  DecodeStateArgs a;
  if (int rc = ds_fill("rv_decode_advance", a, token, len, (int*)budget, done, (int*)pre_off, (int*)pre_len, own_off, eos_ids, n_eos,
                       out_tokens, seen_ids, u_table, ld_t, S, T, tok_in, pos, dst, pre_len_eff, own_len, u_next))
    return rc;
  return launch<decode_advance_kernel>(0, dim3((S + DS_THREADS - 1) / DS_THREADS), dim3(DS_THREADS), stream, a);
}

extern "C" int rv_decode_admit(const int* slots, const int* new_pre_off, const int* new_pre_len, const int* new_budget, int n,
                               const int* token, int* len, int* budget, int* done, int* pre_off, int* pre_len, const int* own_off,
                               const int* eos_ids, int n_eos, int* out_tokens, int* seen_ids, const float* u_table, long ld_t, int S,
                               int T, int* tok_in, int* pos, int* dst, int* pre_len_eff, int* own_len, float* u_next, void* stream) {
  const char* who = "rv_decode_admit";
  DecodeStateArgs a;
  if (int rc = ds_fill(who, a, token, len, budget, done, pre_off, pre_len, own_off, eos_ids, n_eos, out_tokens, seen_ids, u_table,
                       ld_t, S, T, tok_in, pos, dst, pre_len_eff, own_len, u_next))
    return rc;
  RV_REQUIRE_AS(who, n >= 1 && n <= DS_MAX_ADMIT, "1 <= n <= 64 slots per call");
  RV_REQUIRE_AS(who, slots && new_pre_off && new_pre_len && new_budget, "NULL host list");
  DecodeAdmitList q;
  q.n = n;
  for (int i = 0; i < n; ++i) {
    RV_REQUIRE_AS(who, slots[i] >= 0 && slots[i] < S, "slot index outside [0, S)");
    for (int k = 0; k < i; ++k) RV_REQUIRE_AS(who, slots[k] != slots[i], "a slot is listed twice");
    RV_REQUIRE_AS(who, new_budget[i] >= 1 && new_budget[i] <= T, "budget outside [1, T]");
    RV_REQUIRE_AS(who, new_pre_off[i] >= 0 && new_pre_len[i] >= 0, "negative prompt span");
    q.slot[i] = slots[i], q.pre_off[i] = new_pre_off[i], q.pre_len[i] = new_pre_len[i], q.budget[i] = new_budget[i];
  }
  for (int i = n; i < DS_MAX_ADMIT; ++i) q.slot[i] = q.pre_off[i] = q.pre_len[i] = q.budget[i] = 0;
  return launch<decode_admit_kernel>(0, dim3(n), dim3(DS_THREADS), stream, a, q);
}
