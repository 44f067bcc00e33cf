// attn_fwd3_kernel - forward attention, head dim 128, SOFTWARE-PIPELINED INSIDE A WAVE (round 6; VERDICT r5 next 1).
// STATUS: correct (tests/test_kernels_gpu.py::test_attn_fwd3_matches_reference), 12 - 19 % SLOWER than version 2 and therefore NOT the
// default (rv_set_attn_fwd_version(3) / RV_ATTN_FWD=3 select it): profiles/r06_attn_fwd3_negative_result.log has the numbers and the
// ISA-level reason - a wave alone on its SIMD is issue-bound at hipcc's ~9 non-MFMA instructions per MFMA.
//
// Versions 1-2 (attn_fwd2_kernel) give a wave ONE 32-query block: per key tile it runs S^T (16 MFMAs), the softmax (VALU), then PV
// (16 MFMAs) - a serial chain, so the matrix pipe idles while the wave exponentiates and the only overlap is whatever the SIMD's
// OTHER wave happens to be doing (PMC: matrix pipe busy 0.40; phase stamps: MFMA 2 x 1,024 of 4,650 clocks per tile and SIMD).
// Here a wave owns the SIMD alone (4 waves per workgroup, one workgroup per CU, the whole 512-register file) and carries TWO
// 32-query blocks A and B, offset by half a tile, so that every 16-MFMA phase has the OTHER block's softmax as its VALU filler:
//
//     phase 1   PV_B(i-1)   || softmax_A(i), first part  (mask, row max, lazy-rescale decision, 8 of 32 exponentials)
//     phase 2   S_B(i)      || softmax_A(i), rest        (24 exponentials, bf16 packing, row sums)
//     phase 3   PV_A(i)     || softmax_B(i), first part
//     phase 4   S_A(i+1)    || softmax_B(i), rest
//
// Register plan (hard-numbered accumulator file, helpers in attn_agpr.inc): a[0:127] = O of block A (tiles 0-3) and B (4-7),
// a[128:191] = the 16 Q fragments of the wave's 64 rows, a[192:255] = the 16 K fragments of the current key tile - read from LDS
// ONCE per tile (phase 4) and used by S_A(i+1) and, one phase later, by S_B(i+1): both MFMA operands of every S^T step come from
// the accumulator file.  Architectural VGPRs hold the two score tiles (64), the packed P of both blocks (32) and one ring of V^T
// fragments (32).
// LDS: three K tiles + three V tiles + one scratch tile (112 KB), K tile of stage s at s x 16 KB, V at 48 KB + s x 16 KB, so that with the stage a
// COMPILE-TIME constant (the tile loop is unrolled three times) every LDS address is a lane-constant register + an immediate: no
// address arithmetic in the loop at all (version 2 spent one VALU per fragment read).  One barrier per tile; tile i+2 is fetched
// by LDS-DMA while tile i computes (K pieces in phase 2, V pieces in phase 4, counted vmcnt).
// LAZY RESCALE: exponentials are taken against a per-row reference m_ref that is only raised when a tile's row maximum exceeds it
// by more than 2^8 (wave-uniform vote); then O (read / multiply / write through the accumulator file - expensive, hence lazy), l
// and m_ref are rescaled BEFORE the tile's exponentials (textbook order: nothing exponentiated against the old reference is
// pending, see the schedule above).  out = O / l and lse = (m_ref + log2 l) ln 2 are exact for any reference; P <= 2^8 keeps bf16's
// relative precision.
// Waves do not skip tiles individually (a tile above a wave's diagonal is fully masked: p = 0): the workgroup runs in lockstep at
// its barrier anyway, and it keeps the phase structure regular.

// SCHEDULING CONTRACT.  Every 16-MFMA phase is cut into straight-line PARTS (single basic blocks); inside a part the statement order
// is kept by __builtin_amdgcn_sched_barrier(0) after every slot (MFMA + its fillers).  The only branches of a tile - the element
// masks of a diagonal / boundary tile and the rare rescale - sit BETWEEN parts.  (The first build had them inside the phases: hipcc
// then sank every exponential of a phase behind its last MFMA - sched_barrier binds the machine scheduler inside one block only.
// The second pinned the fillers with empty volatile asm statements: correct, but hipcc puts an s_nop behind EVERY inline-asm
// statement, ~250 issue slots per tile for a wave that has nobody to share its SIMD with.)
struct Fwd3Blk {
  f32x16_t s[2];       // S^T of the block as the MFMAs write it: [key half][register]
  float e[32];         // the same 32 scores as scalars (element i = register i & 15 of key half i >> 4): raw, then s c - m, then p
  bf16x8_t p[4];       // packed P, one fragment per 16-key group
  float m, l;          // reference maximum (log2 units, scaled), running sum
  float neg_m;         // -m (0 while the row is still empty)
  float t0, t1;        // row-maximum chains
  float ps0, ps1;      // partial row sums of the current tile
};

template <int J>
__device__ __forceinline__ void fwd3_max_part(Fwd3Blk& b) {
  const float* x = b.e + 8 * J;
  if constexpr (J == 0) {
    b.t0 = fmaxf(x[0], x[1]);
    b.t1 = fmaxf(x[2], x[3]);
    b.t0 = fmaxf(fmaxf(b.t0, x[4]), x[5]);
    b.t1 = fmaxf(fmaxf(b.t1, x[6]), x[7]);
  } else {
    b.t0 = fmaxf(fmaxf(b.t0, x[0]), x[1]);
    b.t1 = fmaxf(fmaxf(b.t1, x[2]), x[3]);
    b.t0 = fmaxf(fmaxf(b.t0, x[4]), x[5]);
    b.t1 = fmaxf(fmaxf(b.t1, x[6]), x[7]);
  }
}

// The 32 exponentials of a lane, SOFTWARE-PIPELINED over the MFMA slots.  A wave alone on its SIMD issues in order: the chain
// v_fma -> v_exp -> v_add of one element stalls on each result.  Here the three stages of an element sit in three CONSECUTIVE
// slots - step g: F = e <- e c - m for elements 2g, 2g + 1, X = e <- 2^e for 2g - 2, 2g - 1, A = row sum += e for 2g - 4, 2g - 3
// - so every instruction's operand is at least one MFMA old.  Steps 0 - 7 are slots 8 - 15 of the PV phase, steps 8 - 17 slots
// 0 - 9 of the S^T phase that follows (which also packs P).  hipcc's DAG scheduler is free to re-pack the stages inside a part (and
// does); what the source order buys is that the three stages of one element are never FORCED together.
template <int G>
__device__ __forceinline__ void fwd3_exp_step(Fwd3Blk& b, float c) {
  if constexpr (G >= 2 && G <= 17) {
    b.ps0 += b.e[2 * G - 4];
    b.ps1 += b.e[2 * G - 3];
  }
  if constexpr (G >= 1 && G <= 16) {
    b.e[2 * G - 2] = __builtin_amdgcn_exp2f(b.e[2 * G - 2]);
    b.e[2 * G - 1] = __builtin_amdgcn_exp2f(b.e[2 * G - 1]);
  }
  if constexpr (G >= 0 && G <= 15) {
    b.e[2 * G] = fmaf(b.e[2 * G], c, b.neg_m);
    b.e[2 * G + 1] = fmaf(b.e[2 * G + 1], c, b.neg_m);
  }
}

template <int K>
__device__ __forceinline__ void fwd3_pack(Fwd3Blk& b) {
  union { uint32_t u[4]; bf16x8_t v; } r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r.u[j] = pack2bf(b.e[8 * K + 2 * j], b.e[8 * K + 2 * j + 1]);
  b.p[K] = r.v;
}

// scores of the finished S^T phase -> scalars.  The volatile asm redefines the two tiles AFTER everything that precedes it, so no
// consumer of a score can be scheduled into the first four slots of the PV phase (the tiles' last MFMAs are still in the pipe
// there, and inline-asm MFMAs are invisible to hipcc's hazard recogniser).
__device__ __forceinline__ void fwd3_unpack(Fwd3Blk& b) {
#pragma unroll
  for (int i = 0; i < 32; ++i) b.e[i] = b.s[i >> 4][i & 15];
}

// rare path of the lazy rescale: tile T0..T0+3 of the accumulator file, l and the reference
template <int T0>
__device__ __forceinline__ void fwd3_rescale(Fwd3Blk& b, float mt, bool scale_o) {
  const float m_new = fmaxf(b.m, mt);
  const float alpha = (m_new == -INFINITY) ? 1.f : __builtin_amdgcn_exp2f(b.m - m_new);
  b.l *= alpha;
  b.m = m_new;
  b.neg_m = (m_new == -INFINITY) ? 0.f : -m_new;
  if (scale_o) {
    asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");      // (the last MFMA on these tiles issued a phase ago; belt and braces)
    acc_scale<T0 + 0>(alpha);
    acc_scale<T0 + 1>(alpha);
    acc_scale<T0 + 2>(alpha);
    acc_scale<T0 + 3>(alpha);
  }
}

// ---- VALU filler of slot SLOT of a PV phase: first part of block b's softmax.  Slots 0-3 nothing (see fwd3_unpack); slots 4-7 the
// row maximum (the masks were applied between slots 3 and 4, the rescale decision follows slot 7), slots 8-15 exponential steps 0-7.
template <int SLOT>
__device__ __forceinline__ void fwd3_sm_first(Fwd3Blk& b, float c) {
  if constexpr (SLOT >= 4 && SLOT <= 7) fwd3_max_part<SLOT - 4>(b);
  if constexpr (SLOT >= 8) fwd3_exp_step<SLOT - 8>(b, c);
}

// ---- VALU filler of slot SLOT of an S^T phase: exponential steps 8-17, packing, row sums
template <int SLOT>
__device__ __forceinline__ void fwd3_sm_rest(Fwd3Blk& b, float c) {
  fwd3_exp_step<SLOT + 8>(b, c);
  if constexpr (SLOT == 6) fwd3_pack<0>(b);        // elements 0-7: exponentials complete after step 4, 8-15 after step 8, ...
  if constexpr (SLOT == 7) fwd3_pack<1>(b);
  if constexpr (SLOT == 10) fwd3_pack<2>(b);
  if constexpr (SLOT == 11) fwd3_pack<3>(b);
  if constexpr (SLOT == 15) b.l += xhalf_sum(b.ps0 + b.ps1);
}

// the pinned MFMAs (see fwd3_exp_step): slot SLOT of a PV phase / of an S^T phase whose filler is block b's softmax
// the MFMAs of a PV / S^T slot.  (A variant that pinned the slot's softmax scalars through extra "+v" operands of these statements
// was measured and dropped: profiles/r06_attn_fwd3_negative_result.log.)
template <int T, int SLOT>
__device__ __forceinline__ void fwd3_pv_mfma(const bf16x8_t& a, const bf16x8_t& p) {
  // the first MFMA that reads a P fragment waits two states: hipcc may have put the fragment's v_cvt_pk right in front of this
  // statement (VALU write -> MFMA operand read; inline asm is invisible to its hazard recogniser)
  if constexpr ((SLOT & 3) == 0) acc_mfma<T>(a, p);
  else acc_mfma_nn<T>(a, p);
}

// One LDS-DMA piece (1 KiB) of the tile prepared by Fwd3Dma::prepare - branch-free, so that a phase part stays one basic block.
struct Fwd3Dma {
  const char* base;        // wave-uniform: sequence base (+ the tile's row offset when the tile lies inside the sequence)
  uint32_t vo[4];          // per-lane byte offset of this wave's four pieces
  template <int P>
  __device__ __forceinline__ void piece(uint8_t* dst_tile, int wave) const {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(base + vo[P]),
                                     (__attribute__((address_space(3))) void*)(dst_tile + (wave * 4 + P) * 1024), 16, 0, 0);
  }
  // tile at row r0 of the sequence that starts at token tok0 of ``src`` (column block already applied); rows >= L are clamped
  __device__ __forceinline__ void prepare(const TileDma<128, 4>& dma, const char* seq, int r0, int L, int wave) {
    if (r0 + 64 <= L) {
      base = seq + (size_t)(uint32_t)r0 * dma.ldb;
#pragma unroll
      for (int i = 0; i < 4; ++i) vo[i] = dma.voff[i];
    } else {
      base = seq;
      const int lane = threadIdx.x & 63;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = TileDma<128, 4>::piece_row(wave, lane, i);
        vo[i] = (uint32_t)min(r0 + row, L - 1) * dma.ldb + (uint32_t)TileDma<128, 4>::piece_col(row, lane) * 2u;
      }
    }
  }
};

// V^T fragment group KK (4 fragments = 8 transposing reads) of the V tile of stage VS into ring r, ONE asm statement
template <int VS, int KK>
__device__ __forceinline__ void fwd3_vreads(bf16x8_t (&r)[4], const uint32_t (&va)[2][4]) {
  constexpr int imm = VS * 16384 + KK * 16 * 256;
  bf16x4s_t l0, h0, l1, h1, l2, h2, l3, h3;
  asm volatile("ds_read_b64_tr_b16 %0, %8 offset:%16\n\tds_read_b64_tr_b16 %1, %9 offset:%16\n\t"
               "ds_read_b64_tr_b16 %2, %10 offset:%16\n\tds_read_b64_tr_b16 %3, %11 offset:%16\n\t"
               "ds_read_b64_tr_b16 %4, %12 offset:%16\n\tds_read_b64_tr_b16 %5, %13 offset:%16\n\t"
               "ds_read_b64_tr_b16 %6, %14 offset:%16\n\tds_read_b64_tr_b16 %7, %15 offset:%16"
               : "=&v"(l0), "=&v"(h0), "=&v"(l1), "=&v"(h1), "=&v"(l2), "=&v"(h2), "=&v"(l3), "=&v"(h3)
               : "v"(va[0][0]), "v"(va[1][0]), "v"(va[0][1]), "v"(va[1][1]), "v"(va[0][2]), "v"(va[1][2]), "v"(va[0][3]), "v"(va[1][3]), "i"(imm)
               : "memory");
  r[0] = __builtin_shufflevector(l0, h0, 0, 1, 2, 3, 4, 5, 6, 7);
  r[1] = __builtin_shufflevector(l1, h1, 0, 1, 2, 3, 4, 5, 6, 7);
  r[2] = __builtin_shufflevector(l2, h2, 0, 1, 2, 3, 4, 5, 6, 7);
  r[3] = __builtin_shufflevector(l3, h3, 0, 1, 2, 3, 4, 5, 6, 7);
}

// K fragment group G (fragments 4G .. 4G+3: key half j & 1, k step 2G + (j >> 1)) of the K tile of stage KSt into a[192:255]
template <int KSt, int G>
__device__ __forceinline__ void fwd3_kreads(const uint32_t (&ka)[8]) { kgroup_load<G>(ka[2 * G], ka[2 * G + 1], KSt * 16384); }

// Groups [G0, G1) of the PV phase of the block whose O tiles are T0..T0+3 (4 MFMAs per group); ring rA holds group 0 on entry of
// group 0 (requested by the phase before).  One basic block.
template <int T0, int VS, int G0, int G1, class Fill>
__device__ __forceinline__ void fwd3_pv_groups(const bf16x8_t (&p)[4], const uint32_t (&va)[2][4], bf16x8_t (&rA)[4], bf16x8_t (&rB)[4],
                                               Fwd3Blk& pin, Fill&& fill) {
  static_for<G1 - G0>([&](auto kc) {
    constexpr int kk = G0 + decltype(kc)::value;
    bf16x8_t (&cur)[4] = (kk & 1) ? rB : rA;
    bf16x8_t (&nxt)[4] = (kk & 1) ? rA : rB;
    if constexpr (kk < 3) {
      fwd3_vreads<VS, kk + 1>(nxt, va);
      asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
    } else {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_sched_barrier(0);
    static_for<4>([&](auto ec) {
      constexpr int e = decltype(ec)::value;
      fwd3_pv_mfma<T0 + e, kk * 4 + e>(cur[e], p[kk]);
      fill(std::integral_constant<int, kk * 4 + e>{});
      __builtin_amdgcn_sched_barrier(0);
    });
  });
}

// S^T phase: s = K Q_X^T with Q fragments QB..QB+7.  LOADK: the K fragments of stage KSt are read into the accumulator file here
// (groups 0 and 1 were requested by the phase before); otherwise they are already there.  One basic block.
template <int QB, bool LOADK, int KSt, class Fill>
__device__ __forceinline__ void fwd3_phase_s(f32x16_t (&s)[2], const uint32_t (&ka)[8], Fwd3Blk& pin, Fill&& fill) {
  static_for<4>([&](auto gc) {
    constexpr int g = decltype(gc)::value;
    if constexpr (LOADK) {
      if constexpr (g < 2) {
        fwd3_kreads<KSt, g + 2>(ka);
        asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
      } else if constexpr (g == 2) {
        asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    static_for<4>([&](auto jc) {
      constexpr int j = decltype(jc)::value, kt = j & 1, ks = 2 * g + (j >> 1);
      smfma_q<2 * ks + kt, QB + ks, ks == 0>(s[kt]);
      fill(std::integral_constant<int, g * 4 + j>{});
      __builtin_amdgcn_sched_barrier(0);
    });
  });
}

// The PV phase of block `o` (O tiles TO.., packed P in o.p, V stage VS) with the first part of block b's softmax underneath:
//   part 1  slots 0-3    | masks of b (diagonal / boundary tiles only) |
//   part 2  slots 4-7    row maximum                                   | lazy-rescale decision, rare rescale (O tiles TB..) |
//   part 3  slots 8-15   first exponentials; ``extra(slot)`` adds the phase's own LDS / DMA fillers to parts 2 and 3
template <int TO, int VS, int TB, bool CAUSAL, class Extra>
__device__ __forceinline__ void fwd3_phase_pv(const Fwd3Blk& o, Fwd3Blk& b, const uint32_t (&va)[2][4], bf16x8_t (&rA)[4], bf16x8_t (&rB)[4],
                                              const QueryLaneMask<CAUSAL>& qm, bool need_mask, int kb, float c, bool scale_o, Extra&& extra) {
  fwd3_pv_groups<TO, VS, 0, 1>(o.p, va, rA, rB, b, [&](auto) {});
  asm volatile("" : "+v"(b.s[0]), "+v"(b.s[1]));
  if (need_mask) {
    qm.apply(b.s[0], kb);
    qm.apply(b.s[1], kb + 32);
  }
  fwd3_unpack(b);
  fwd3_pv_groups<TO, VS, 1, 2>(o.p, va, rA, rB, b, [&](auto sc) { fwd3_sm_first<decltype(sc)::value>(b, c); });
  {
    const float mt = xhalf_max(fmaxf(b.t0, b.t1)) * c;
    if (__any(mt > b.m + 8.0f)) fwd3_rescale<TB>(b, mt, scale_o);      // the reference lags by more than 2^8
    b.ps0 = 0.f;
    b.ps1 = 0.f;
  }
  fwd3_pv_groups<TO, VS, 2, 4>(o.p, va, rA, rB, b, [&](auto sc) {
    fwd3_sm_first<decltype(sc)::value>(b, c);
    extra(sc);
  });
}

template <bool CAUSAL>
__global__ __launch_bounds__(256, 1) void attn_fwd3_kernel(const bf16_t* __restrict__ qkv, long ld, int q_col0, int k_col0, int v_col0,
                                                           bf16_t* __restrict__ out, long ldo, float* __restrict__ lse, int Lmax, int H,
                                                           int nx, float scale, const int* __restrict__ seg_sh,
                                                           const int* __restrict__ seg_e1, int kv_group,
                                                           const int* __restrict__ row_off, const int* __restrict__ row_len) {
  constexpr int HD = 128, TILE = 64 * HD * 2, BQ = 256, VBASE = 3 * TILE;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 31, half = lane >> 5;
  int bx, h, s;
  attn_block_coords(nx, H, (int)gridDim.x / ((nx & 0xffff) * H), bx, h, s);
  const int L = row_len ? row_len[s] : Lmax;
  const long tok0 = row_off ? (long)row_off[s] : (long)s * Lmax;
  const int nqb = (L + BQ - 1) / BQ;
  if (varlen_done(bx, nqb, CAUSAL && !((nx >> 21) & 1))) return;
  const int sh = seg_sh ? seg_sh[s] : 0, e1 = seg_e1 ? seg_e1[s] : 0;
  const float c = scale * LOG2E;

  TileDma<HD, 4> dma;
  dma.init(wave, lane, ld);
  const uint32_t sbase = lds_addr_of(smem);
  uint32_t ka[8], va[2][4];
  {
    TrOffsets<HD> tro;
    tro.init(lane);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) ka[ks] = sbase + kvtile_off<HD>(fr, 2 * ks + half);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) va[u][e] = sbase + VBASE + tro.off[u][e];
  }
  const bf16_t* kbase = qkv + k_col0 + (h / kv_group) * HD;
  const bf16_t* vbase = qkv + v_col0 + (h / kv_group) * HD;
  // the V tile of stage 2 is multiplied by P = 0 before anything was fetched into it (phase 1 of the first tile): make it finite
  {
    const u32x4_t z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < TILE / (256 * 16); ++i) *(u32x4_t*)(smem + VBASE + 2 * TILE + (i * 256 + tid) * 16) = z;
  }

  int blk_first, blk_second;
  pair_blocks<false, BQ>(bx, nqb, L, sh, e1, lane, CAUSAL && ((nx >> 20) & 1), CAUSAL && ((nx >> 21) & 1), blk_first, blk_second);
  const int npass = CAUSAL ? 2 : 1;
  for (int pass = 0; pass < npass; ++pass) {
    const int qb = (pass == 0) ? blk_first : blk_second;
    if (qb < 0) break;
    const int q0 = qb * BQ, q0w = q0 + wave * 64;
    const int qA = q0w + fr, qB = qA + 32;
    QueryLaneMask<CAUSAL> qmA, qmB;
    qmA.init(qA, L, sh, e1);
    qmB.init(qB, L, sh, e1);

    const int kv_end = CAUSAL ? min(L, q0 + BQ) : L;
    const int nt = (kv_end + 63) / 64;
    int skip_lo = nt, skip_n = 0;
    if (q0 >= e1 && e1 > sh) {
      const int lo = (sh + 63) >> 6, hi = e1 >> 6;
      if (hi > lo) { skip_lo = lo; skip_n = hi - lo; }
    }
    const int nte = nt - skip_n;
    const char* const kseq = (const char*)(kbase + tok0 * ld);
    const long v_minus_k = (const char*)vbase - (const char*)kbase;
    auto tile_k0 = [&](int i) { return ((i < skip_lo) ? i : i + skip_n) * 64; };

    // ---- prologue: tiles 0 and 1 by LDS-DMA, the 16 Q fragments straight into the accumulator file, O = 0
    asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");          // second pass: the read-out of the first one is complete
    __builtin_amdgcn_s_barrier();                              // ... and every wave is done with the first pass's tiles
    dma.issue(kbase, ld, tok0, tile_k0(0), L, smem, wave);
    dma.issue(vbase, ld, tok0, tile_k0(0), L, smem + VBASE, wave);
    if (nte > 1) {
      dma.issue(kbase, ld, tok0, tile_k0(1), L, smem + TILE, wave);
      dma.issue(vbase, ld, tok0, tile_k0(1), L, smem + VBASE + TILE, wave);
    }
    {
      const bf16_t* qpA = qkv + (tok0 + min(qA, L - 1)) * ld + q_col0 + h * HD + 8 * half;
      const bf16_t* qpB = qkv + (tok0 + min(qB, L - 1)) * ld + q_col0 + h * HD + 8 * half;
      static_for<8>([&](auto kc) {
        constexpr int ks = decltype(kc)::value;
        frag_load<ks>(qpA + 16 * ks);
        frag_load<8 + ks>(qpB + 16 * ks);
      });
    }
    static_for<8>([&](auto tc) { acc_zero<decltype(tc)::value>(); });
    Fwd3Blk A, B;
    A.m = B.m = -INFINITY;
    A.l = B.l = 0.f;
    A.neg_m = B.neg_m = 0.f;
    A.ps0 = A.ps1 = B.ps0 = B.ps1 = 0.f;
    A.t0 = A.t1 = B.t0 = B.t1 = -INFINITY;
#pragma unroll
    for (int k = 0; k < 32; ++k) A.e[k] = B.e[k] = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) B.p[k] = bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
    bf16x8_t rA[4], rB[4];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    // S_A(0): its own K reads, nothing to overlap with yet
    fwd3_kreads<0, 0>(ka);
    fwd3_kreads<0, 1>(ka);
    fwd3_phase_s<0, true, 0>(A.s, ka, B, [&](auto) {});
    asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");
    fwd3_vreads<2, 0>(rA, va);                                  // group 0 of "V(-1)" (zeros x P = 0) for the first phase 1

    // ---- one key tile; ST = i % 3 = the LDS stage of tile i
    auto body = [&](auto stc, int i) {
      constexpr int ST = decltype(stc)::value, SP = (ST + 2) % 3, SN = (ST + 1) % 3;
      const int k0 = tile_k0(i);
      const bool maskA = (k0 + 63 >= L) || (CAUSAL && k0 + 63 > q0w) || (q0w + 31 >= e1 && k0 + 63 >= sh && k0 < e1);
      const bool maskB = (k0 + 63 >= L) || (CAUSAL && k0 + 63 > q0w + 32) || (q0w + 63 >= e1 && k0 + 63 >= sh && k0 < e1);
      const bool more = i + 2 < nte;
      // tile i + 2 -> stage SP; past the last tile the pieces re-fetch tile 0 into a scratch tile behind the ring (branch-free phases)
      Fwd3Dma dk, dv;
      {
        const int kn = more ? tile_k0(i + 2) : 0;
        dk.prepare(dma, kseq, kn, L, wave);
        dv.base = dk.base + v_minus_k;
#pragma unroll
        for (int p_ = 0; p_ < 4; ++p_) dv.vo[p_] = dk.vo[p_];
      }
      uint8_t* const dstk = more ? smem + SP * TILE : smem + 6 * TILE;
      uint8_t* const dstv = more ? smem + VBASE + SP * TILE : smem + 6 * TILE;
      // phase 1: PV_B(i-1) on V(stage SP) || softmax_A(i) first part
      fwd3_phase_pv<4, SP, 0, CAUSAL>(B, A, va, rA, rB, qmA, maskA, k0 + 4 * half, c, i > 0, [&](auto) {});
      // every wave is done with stage SP (K(i-1) since phase 2 of the last tile, V(i-1) now) -> tile i+2 may land there; and the
      // K tile of i+1 (pieces issued a whole tile ago) becomes visible to all waves for phase 4
      // (pieces are issued in EVERY tile - past the end into the scratch tile - so "all but the newest four" is always the right count)
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      // phase 2: S_B(i) (K fragments already in a[192:255]) || softmax_A(i) rest; K pieces of tile i+2; V(i) group 0 requested
      fwd3_phase_s<8, false, ST>(B.s, ka, A, [&](auto sc) {
        constexpr int sl = decltype(sc)::value;
        fwd3_sm_rest<sl>(A, c);
        if constexpr ((sl & 3) == 1) dk.template piece<(sl >> 2)>(dstk, wave);
        if constexpr (sl == 13) fwd3_vreads<ST, 0>(rA, va);
      });
      // phase 3: PV_A(i) on V(stage ST) || softmax_B(i) first part; K(i+1) groups 0, 1 requested at the end
      fwd3_phase_pv<0, ST, 4, CAUSAL>(A, B, va, rA, rB, qmB, maskB, k0 + 4 * half, c, i > 0, [&](auto sc) {
        constexpr int sl = decltype(sc)::value;
        if constexpr (sl == 13) fwd3_kreads<SN, 0>(ka);
        if constexpr (sl == 14) fwd3_kreads<SN, 1>(ka);
      });
      // phase 4: S_A(i+1) from K(stage SN) || softmax_B(i) rest; V pieces of tile i+2; V(i) group 0 requested for the next phase 1
      fwd3_phase_s<0, true, SN>(A.s, ka, B, [&](auto sc) {
        constexpr int sl = decltype(sc)::value;
        fwd3_sm_rest<sl>(B, c);
        if constexpr ((sl & 3) == 1) dv.template piece<(sl >> 2)>(dstv, wave);
        if constexpr (sl == 13) fwd3_vreads<ST, 0>(rA, va);
      });
    };
    // One copy of the tile body per LDS stage, selected per tile (a scalar compare + branch per 2,000-cycle tile).  The first build
    // unrolled the loop three times with a two-body tail: blocks with nte % 3 == 2 then came out with garbage in the B rows of
    // random waves, non-deterministically (GPU box, r06); extra waits, barriers and wait states at every phase boundary changed
    // nothing, this form is clean - the eight-body version put register copies of values that are still in flight (MFMA results,
    // LDS reads issued by inline asm, both invisible to hipcc) on some loop-exit edge.  Keep ONE back-edge.
    for (int i = 0; i < nte; ++i) {
      const int st = i % 3;
      if (st == 0) body(std::integral_constant<int, 0>{}, i);
      else if (st == 1) body(std::integral_constant<int, 1>{}, i);
      else body(std::integral_constant<int, 2>{}, i);
    }
    const int rem = nte % 3;
    // ---- epilogue: PV_B(last) on the stage of the last tile
    if (rem == 0) fwd3_pv_groups<4, 2, 0, 4>(B.p, va, rA, rB, A, [&](auto) {});
    else if (rem == 1) fwd3_pv_groups<4, 0, 0, 4>(B.p, va, rA, rB, A, [&](auto) {});
    else fwd3_pv_groups<4, 1, 0, 4>(B.p, va, rA, rB, A, [&](auto) {});
    // the last MFMAs have left the pipe before the read-out; no LDS-DMA piece (the last tiles' go to the scratch tile) may still be
    // in flight when the workgroup ends and its LDS is handed to another one
    asm volatile("s_waitcnt vmcnt(0)\n\ts_nop 15\n\ts_nop 15\n\ts_nop 7" ::: "memory");

    // ---- read-out: out = O / l, lse = (m_ref + log2 l) ln 2
    auto store_block = [&](auto tb, int q, float m_ref, float l_run) {
      constexpr int T0 = decltype(tb)::value;
      if (q < L) {
        const float inv = 1.f / l_run;
        bf16_t* op = out + (tok0 + q) * ldo + h * HD;
        static_for<4>([&](auto ec) {
          constexpr int e = decltype(ec)::value;
          f32x16_t o;
          acc_read<T0 + e>(o);
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            uint2 w;
            w.x = pack2bf(o[rg * 4 + 0] * inv, o[rg * 4 + 1] * inv);
            w.y = pack2bf(o[rg * 4 + 2] * inv, o[rg * 4 + 3] * inv);
            *(uint2*)(op + e * 32 + rg * 8 + 4 * half) = w;
          }
        });
        if (half == 0) lse[((long)s * H + h) * Lmax + q] = (m_ref + log2f(l_run)) * LN2;
      }
    };
    store_block(std::integral_constant<int, 0>{}, qA, A.m, A.l);
    store_block(std::integral_constant<int, 4>{}, qB, B.m, B.l);
  }  // pass
}
