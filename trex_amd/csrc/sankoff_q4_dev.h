// The Q <= 4 one-site-per-lane Sankoff kernels' device code (sankoff.hip: the
// 36 sankoff_kernel instantiations; sankoff_fused4.hip: the Q = 4 softmin
// fused kernel, which runs its own loops on the same helpers and tables and
// calls sankoff_body for the cost matrices it does not cover).
#pragma once

#include <hip/hip_runtime.h>

#include "sankoff_dev.h"
#include "trex_common.h"

namespace trex {

namespace {

// one site's leaf code / ancestral state (int8 in memory); the __restrict__
// tells the compiler that these bytes alias no DP row or LDS slot
__device__ __forceinline__ int ld_code(const int8_t* __restrict__ p) { return *p; }
__device__ __forceinline__ void st_code(int8_t* __restrict__ p, int c) { *p = (int8_t)c; }

// --------------------------------------------------------------------------
// cost matrix in SGPRs.  MODE: kHard (min-plus), kSoftK (factored softmin,
// K[i][j] = exp(-(C[i][j]-cmin)/tau) in SGPRs), kSoftDirect (per-row
// stabilised softmin, used when range(C)/tau > 40 would underflow K).
// --------------------------------------------------------------------------

template <int Q>
struct Coef {
  float c[Q][Q];
  float k[Q][Q];
  float cmin;
};


template <int Q>
__device__ __forceinline__ void cost_range(const float* __restrict__ cost_, float& cmin,
                                           float& cmax) {
  const cptr<float> cost = as_const(cost_);
  cmin = INFINITY;
  cmax = -INFINITY;
#pragma unroll
  for (int q = 0; q < Q * Q; ++q) {
    const float v = cost[q];
    cmin = fminf(cmin, v);
    cmax = fmaxf(cmax, v);
  }
  cmin = uniform(cmin);
  cmax = uniform(cmax);
}

// C == C^T (then K == K^T), wave-uniform
template <int Q>
__device__ __forceinline__ bool cost_symmetric(const float* __restrict__ cost_) {
  const cptr<float> cost = as_const(cost_);
  bool sym = true;
#pragma unroll
  for (int i = 0; i < Q; ++i)
#pragma unroll
    for (int j = i + 1; j < Q; ++j) sym = sym && cost[i * Q + j] == cost[j * Q + i];
  return sym;
}

template <int Q, int MODE>
__device__ __forceinline__ void load_coef(const float* __restrict__ cost_, float a, Coef<Q>& cf) {
  float cmax;
  cost_range<Q>(cost_, cf.cmin, cmax);
  const cptr<float> cost = as_const(cost_);
#pragma unroll
  for (int i = 0; i < Q; ++i)
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const float v = cost[i * Q + j];
      cf.c[i][j] = v;
      if constexpr (MODE == kSoftK) cf.k[i][j] = uniform(fast_exp2((cf.cmin - v) * a));
    }
}

// --------------------------------------------------------------------------
// child value D_c (leaf row / LDS slot / dp row / 1e5 sentinel row)
// --------------------------------------------------------------------------
// LDS slot stack: [slot][lane][Q] -- each lane's vector is contiguous, so a
// slot access is one ds_read / ds_write of Q floats (b128 at Q = 4).
template <int N>
__device__ __forceinline__ void lds_vec_get(const float* p, float (&o)[N]) {
  if constexpr (N % 4 == 0) {
#pragma unroll
    for (int t = 0; t < N / 4; ++t) {
      const float4 v = reinterpret_cast<const float4*>(p)[t];
      o[4 * t] = v.x; o[4 * t + 1] = v.y; o[4 * t + 2] = v.z; o[4 * t + 3] = v.w;
    }
  } else if constexpr (N % 2 == 0) {
#pragma unroll
    for (int t = 0; t < N / 2; ++t) {
      const float2 v = reinterpret_cast<const float2*>(p)[t];
      o[2 * t] = v.x; o[2 * t + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int t = 0; t < N; ++t) o[t] = p[t];
  }
}

template <int N>
__device__ __forceinline__ void lds_vec_put(float* p, const float (&o)[N]) {
  if constexpr (N % 4 == 0) {
#pragma unroll
    for (int t = 0; t < N / 4; ++t)
      reinterpret_cast<float4*>(p)[t] = make_float4(o[4 * t], o[4 * t + 1], o[4 * t + 2], o[4 * t + 3]);
  } else if constexpr (N % 2 == 0) {
#pragma unroll
    for (int t = 0; t < N / 2; ++t) reinterpret_cast<float2*>(p)[t] = make_float2(o[2 * t], o[2 * t + 1]);
  } else {
#pragma unroll
    for (int t = 0; t < N; ++t) p[t] = o[t];
  }
}

// (both go through a local copy: the compiled kernels are the ones measured in
// PERFLOG.md only in this form, see kSites)
template <int Q>
__device__ __forceinline__ void lds_get(const float* lds, int slot, int lane, float (&d)[Q]) {
  float buf[Q];
  lds_vec_get<Q>(lds + (slot * kWave + lane) * Q, buf);
#pragma unroll
  for (int j = 0; j < Q; ++j) d[j] = buf[j];
}

template <int Q>
__device__ __forceinline__ void lds_put(float* lds, int slot, int lane, const float (&d)[Q]) {
  float buf[Q];
#pragma unroll
  for (int j = 0; j < Q; ++j) buf[j] = d[j];
  lds_vec_put<Q>(lds + (slot * kWave + lane) * Q, buf);
}

// C[i][code] from SGPR operands (code in [0, Q)); bit-tree select on SSA values
template <int Q>
__device__ __forceinline__ float pick(const float (&row)[Q], int code) {
  float r[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = row[j < Q ? j : 0];
  const bool b0 = (code & 1) != 0;
  const float lo = b0 ? r[1] : r[0];
  if constexpr (Q == 2) return lo;
  if constexpr (Q == 3) return (code & 2) ? r[2] : lo;
  const float hi = b0 ? r[3] : r[2];
  return (code & 2) ? hi : lo;
}

// Cache policy (the buffer instructions' aux bits, 2 = nt; bld_row / bst_row,
// sankoff_dev.h) of the DP-row accesses.  Each value won its A/B (PERFLOG.md):
constexpr int kAuxFwdRow = 2;     // forward-only row stores stream: C4 forward 620 -> 560 us
constexpr int kAuxAdjRow = 2;     // adjoint-only row reads stream: C4 adjoint 588 -> ~577 us
constexpr int kAuxMarg = 2;       // marginal stores stream (never re-read by the kernel)
constexpr int kAuxFusedRow = 0;   // fused stores stay temporal: all-nt, 128-tree shard 128 -> 135 us
constexpr int kAuxFusedLoad = 2;  // fused re-reads (read once, then dead): 929-934 -> 903-911 us
constexpr int kAuxCherryRow = 2;  // fused deferred-cherry rows (never re-read): shard 134 -> 128 us
constexpr int kAuxLeaf = 0;       // leaf-tile prefetch loads: nt made the forward 521 -> 643 us
// waves per SIMD asked of the compiler (amdgpu_waves_per_eu), per phase
constexpr int kFwdWpe = 6;    // forward-only (LDS-bound at C4)
constexpr int kAdjWpe = 5;    // adjoint-only: 6 spills (235 vs 171 us), 7 too (fused 1 015 -> 1 077)
constexpr int kFusedWpe = 5;  // fused: 6 or 4 waves measured 958-1 155 vs 934-943 us
constexpr int kFusedWpeMax = 8;
// adjoint DP-row prefetch depth (steps): 2 -> 3 C4 fused 1 015 -> 988 us, 4 no further gain
constexpr int kAdjRing = 3;

// s_i = sum_j K_ij u_j for every parent state i.  SYM (K = K^T, symmetric
// C): s_i = sum_j K_ji u_j, accumulated over j with the row pairs (K_j,2p,
// K_j,2p+1) already in SGPRs -- Q / 2 v_pk_fma_f32 per j (8 at Q = 4) instead
// of a pair-wise dot per i (12)
template <int Q, bool SYM>
__device__ __forceinline__ void kvec(const Coef<Q>& cf, const float (&u)[Q], float (&sv)[Q]) {
  if constexpr (SYM && Q % 2 == 0) {
    f2 acc[Q / 2];
#pragma unroll
    for (int p = 0; p < Q / 2; ++p) acc[p] = pk(cf.k[0][2 * p], cf.k[0][2 * p + 1]) * pk(u[0], u[0]);
#pragma unroll
    for (int j = 1; j < Q; ++j)
#pragma unroll
      for (int p = 0; p < Q / 2; ++p)
        acc[p] = __builtin_elementwise_fma(pk(cf.k[j][2 * p], cf.k[j][2 * p + 1]), pk(u[j], u[j]), acc[p]);
#pragma unroll
    for (int p = 0; p < Q / 2; ++p) {
      sv[2 * p] = acc[p].x;
      sv[2 * p + 1] = acc[p].y;
    }
  } else {
#pragma unroll
    for (int i = 0; i < Q; ++i) sv[i] = kdot<Q>(cf.k[i], u);
  }
}

// --------------------------------------------------------------------------
// message M_c[i] = min_j / smin_j (C[i][j] + D_c[j])      (sankoff.py:67-68)
// --------------------------------------------------------------------------
template <int Q, int MODE, bool SYM = false>
__device__ __forceinline__ void message(const Coef<Q>& cf, float a, float bcoef,
                                        const float (&d)[Q], float (&m)[Q]) {
  if constexpr (MODE == kHard) {
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      float v = cf.c[i][0] + d[0];
#pragma unroll
      for (int j = 1; j < Q; ++j) v = fminf(v, cf.c[i][j] + d[j]);
      m[i] = v;
    }
  } else if constexpr (MODE == kSoftK) {
    float md = d[0];
#pragma unroll
    for (int j = 1; j < Q; ++j) md = fminf(md, d[j]);
    const float mda = md * a;
    float u[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) u[j] = fast_exp2(fmaf(-d[j], a, mda));
    const float base = md + cf.cmin;
    float sv[Q];
    kvec<Q, SYM>(cf, u, sv);
#pragma unroll
    for (int i = 0; i < Q; ++i) m[i] = fmaf(-bcoef, fast_log2(sv[i]), base);
  } else {
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      float x[Q];
      float mn = INFINITY;
#pragma unroll
      for (int j = 0; j < Q; ++j) {
        x[j] = cf.c[i][j] + d[j];
        mn = fminf(mn, x[j]);
      }
      float acc = 0.0f;
#pragma unroll
      for (int j = 0; j < Q; ++j) acc += fast_exp2((mn - x[j]) * a);
      m[i] = fmaf(-bcoef, fast_log2(acc), mn);
    }
  }
}

// factored-softmin edge adjoint in two halves.  softk_weights: what depends
// on the child's D alone (u_j = exp((min D - D_j)/tau), 1 / s_i, s = K u);
// softk_edge: the parent cotangent applied to them.  A deferred cherry's D is
// a function of its two leaf codes, so its first half is a table lookup
// (TREX_PAIR_TABLES).
template <int Q, bool SYM>
__device__ __forceinline__ void softk_weights(const Coef<Q>& cf, float a, const float (&d)[Q],
                                              float (&u)[Q], float (&rs)[Q]) {
  float md = d[0];
#pragma unroll
  for (int j = 1; j < Q; ++j) md = fminf(md, d[j]);
  const float mda = md * a;
#pragma unroll
  for (int j = 0; j < Q; ++j) u[j] = fast_exp2(fmaf(-d[j], a, mda));
  float sv[Q];
  kvec<Q, SYM>(cf, u, sv);
#pragma unroll
  for (int i = 0; i < Q; ++i) rs[i] = __builtin_amdgcn_rcpf(sv[i]);
}

template <int Q>
__device__ __forceinline__ void softk_edge(const Coef<Q>& cf, const float (&u)[Q],
                                           const float (&rs)[Q], const float (&g)[Q],
                                           float (&acc)[Q][Q], float (&gc)[Q]) {
  float r[Q];
#pragma unroll
  for (int i = 0; i < Q; ++i) r[i] = g[i] * rs[i];
#pragma unroll
  for (int i = 0; i < Q; ++i) axpy<Q>(acc[i], r[i], u);
  // t[j] = sum_i r_i K[i][j] (row pairs of K), gc = u * t
  float t[Q];
#pragma unroll
  for (int j = 0; j < Q; ++j) t[j] = r[0] * cf.k[0][j];
#pragma unroll
  for (int i = 1; i < Q; ++i) axpy<Q>(t, r[i], cf.k[i]);
#pragma unroll
  for (int j = 0; j < Q; ++j) gc[j] = u[j] * t[j];
}

// --------------------------------------------------------------------------
// adjoint of one child message: acc[i][j] += gbar[i] w[i][j];
// gc[j] = sum_i gbar[i] w[i][j]   (w = tie-averaged argmin or softmax weights)
// In the factored softmin acc holds sum r_i u_j; the K[i][j] factor is
// applied once in the final reduction.
// --------------------------------------------------------------------------
template <int Q, int MODE, bool SYM = false>
__device__ __forceinline__ void message_adjoint(const Coef<Q>& cf, float a, const float (&d)[Q],
                                                const float (&g)[Q], float (&acc)[Q][Q],
                                                float (&gc)[Q]) {
  if constexpr (MODE == kHard) {
#pragma unroll
    for (int j = 0; j < Q; ++j) gc[j] = 0.0f;
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      float x[Q];
      float mn = cf.c[i][0] + d[0];
      x[0] = mn;
#pragma unroll
      for (int j = 1; j < Q; ++j) {
        x[j] = cf.c[i][j] + d[j];
        mn = fminf(mn, x[j]);
      }
      float cnt = 0.0f;
#pragma unroll
      for (int j = 0; j < Q; ++j) cnt += (x[j] == mn) ? 1.0f : 0.0f;
      const float r = g[i] / cnt;
#pragma unroll
      for (int j = 0; j < Q; ++j) {
        const float w = (x[j] == mn) ? r : 0.0f;
        acc[i][j] += w;
        gc[j] += w;
      }
    }
  } else if constexpr (MODE == kSoftK) {
    float u[Q], rs[Q];
    softk_weights<Q, SYM>(cf, a, d, u, rs);
    softk_edge<Q>(cf, u, rs, g, acc, gc);
  } else {
#pragma unroll
    for (int j = 0; j < Q; ++j) gc[j] = 0.0f;
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      float x[Q];
      float mn = INFINITY;
#pragma unroll
      for (int j = 0; j < Q; ++j) {
        x[j] = cf.c[i][j] + d[j];
        mn = fminf(mn, x[j]);
      }
      float e[Q];
      float sm = 0.0f;
#pragma unroll
      for (int j = 0; j < Q; ++j) {
        e[j] = fast_exp2((mn - x[j]) * a);
        sm += e[j];
      }
      const float r = g[i] * __builtin_amdgcn_rcpf(sm);
#pragma unroll
      for (int j = 0; j < Q; ++j) {
        const float w = r * e[j];
        acc[i][j] += w;
        gc[j] += w;
      }
    }
  }
}

// root: score and cotangent of the per-site score      (sankoff.py:187)
template <int Q, bool SOFT>
__device__ __forceinline__ void root_score(const float (&d)[Q], float a, float bcoef,
                                           bool hard_root, float& score, float (&w)[Q]) {
  float mn = d[0];
#pragma unroll
  for (int i = 1; i < Q; ++i) mn = fminf(mn, d[i]);
  if (!SOFT || hard_root) {
    float cnt = 0.0f;
#pragma unroll
    for (int i = 0; i < Q; ++i) cnt += (d[i] == mn) ? 1.0f : 0.0f;
    const float r = 1.0f / cnt;
#pragma unroll
    for (int i = 0; i < Q; ++i) w[i] = (d[i] == mn) ? r : 0.0f;
    score = mn;
  } else {
    float sm = 0.0f;
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      w[i] = fast_exp2((mn - d[i]) * a);
      sm += w[i];
    }
    const float r = __builtin_amdgcn_rcpf(sm);
#pragma unroll
    for (int i = 0; i < Q; ++i) w[i] *= r;
    score = fmaf(-bcoef, fast_log2(sm), mn);
  }
}


// --------------------------------------------------------------------------
// Unified Sankoff kernel: PHASE 1 = forward, 2 = adjoint, 3 = both (fused).
//
// One wave per workgroup = 64 consecutive sites of one tree.  LDS holds
//   [slots][64][Q] f32  live D vectors (forward) / cotangents (adjoint)
//   [nl][64]       i8   the tile's leaf states (prologue prefetch)
// Leaf and sentinel children are lookups in per-code tables (message and
// adjoint weights; exact closed forms C[i][code] / one-hot when the 1e5
// sentinel dominates), i.e. no transcendental for half of all children.
// --------------------------------------------------------------------------
struct KArgs {
  const int4* steps;
  const int8_t* leaves;
  const float* cost;
  int n_int, nl, L, tiles, B, n_slots;
  float a, bcoef;
  int hard_root;
  float* dp;            // [B][n_int][L][Q] site-major (fwd writes / adjoint reads)
  float* site_score;    // [B][L] or null
  float* tree_score;    // [B]
  const float* dts;     // [B] or null
  float* marg;          // [B][n_int][L][Q] or null
  int8_t* anc;          // [B][n_int][L] or null
  float* d_cost;        // [Q][Q]
  double* part_tree;    // [B*tiles] per-item score partials
  double* part_dc;      // [Q*Q][B*tiles] per-item dC partials
  int nblocks;          // B * tiles work items (ragged: sum of per-tree tiles)
  // ragged batches (null for uniform batches): per-tree records and the
  // work-item -> tree table of the ragged plan (trex_ragged_plan_build)
  const int* rmeta;     // [B][kRaggedMeta]
  const int* ritem;     // [nblocks] tree of each work item
};

// host: the Q <= 4 kernels' arguments of a call.  A uniform batch has one item
// per (tree, 64 sites) and its partials behind the workspace's counters; a
// ragged one the plan's items and its partials at the workspace's start.
inline int q4_tiles(int L) { return (L + kWave - 1) / kWave; }
inline int64_t q4_counters_bytes(int B) { return ((int64_t)4 * (B + 1) + 255) / 256 * 256; }
inline KArgs q4_args(const SankoffCall& c) {
  const bool ragged = c.rmeta != nullptr;
  const int tiles = ragged ? 0 : q4_tiles(c.L);
  KArgs A;
  A.nblocks = ragged ? (int)c.items : c.B * tiles;
  fill_common(A, c, ragged ? 0 : c.ni, c.L, tiles, A.nblocks,
              ragged ? 0 : q4_counters_bytes(c.B));
  A.steps = reinterpret_cast<const int4*>(c.steps);
  A.n_slots = c.n_slots;
  A.tree_score = c.tree_score;
  A.d_cost = c.d_cost;
  A.rmeta = c.rmeta;
  A.ritem = c.ritem;
  return A;
}

// ragged plan per-tree record (ints): steps offset (in steps), n_int, n_leaves,
// L, first site (site_score offset), first work item, leaf byte offset (lo, hi),
// row-site offset of the tree's DP rows (lo, hi; x Q floats), 2 spare


// LDS map (floats): [0, 128) leaf tables, one row per leaf code (code Q =
// missing leaf / all-1e5 sentinel row): T[code][i] = the child's message at
// 0, W[code][i][j] = its adjoint weight (divided by K_ij in the factored
// form) at kWTab -- both depend on the code only, so every leaf / sentinel
// child is a table lookup in both sweeps; then the slot stack
// [max(n_slots, 1)][64][Q], then the leaf tile [nl][64] i8 (raw
// codes, normalised to [0, Q] at use).  The root's cotangent goes to slot 0:
// it is written after the forward has consumed every slot and read by the
// first reverse step (always the root's), before any child cotangent is
// written, and slots are lane-private (a dedicated root slot cost 1 KiB per
// wave: 24 -> 29 waves per CU at C4's 3 slots).
//
// Pair tables (TREX_PAIR_TABLES): a deferred cherry's D is T[c0] + T[c1], a
// function of its two leaf codes, so everything the sweeps compute from it is
// one of (Q + 1)^2 <= 25 vectors, indexed p = c0 (Q + 1) + c1: TM[p][i] its
// message to the parent (every mode), TU[p][j] / TR[p][i] the u_j and 1 / s_i
// of the parent -> cherry edge adjoint (factored softmin).  Built once per
// wave from the same helpers the lanes run, so a lookup is bitwise what the
// lane would compute.  Adjoint-bearing kernels keep them after the leaf tables
// (1 200 B more per wave, their occupancy comes from their registers); the
// forward-only kernel (LDS-bound at C4) has no W and keeps TM over its region,
// at kPairFwd, so its LDS is unchanged.
#ifndef TREX_PAIR_TABLES
#define TREX_PAIR_TABLES 1  // 0: cherries compute their message / edge weights per site
#endif
constexpr bool kPairTables = TREX_PAIR_TABLES != 0;
constexpr int kLeafTabFloats = 128;
constexpr int kWTab = 32;  // (Q + 1) Q <= 20 message floats precede the weights
constexpr int kPairFloats = 100;  // (Q + 1)^2 Q at Q = 4
constexpr int kPairFwd = 28;      // forward-only: TM at [28, 128)
// table floats ahead of the slot stack
constexpr int tab_floats(int phase) {
  return kLeafTabFloats + ((kPairTables && phase != 1) ? 3 * kPairFloats : 0);
}
// The fused Q = 4 kernel (sankoff_fused4.hip) runs workgroups of kF4Waves
// waves, one item each, on one copy of the tables above: [tab_floats(3)], then
// every wave's own slot stack and leaf tile (f4_wave_lds).  1 712 B of tables
// per workgroup instead of per wave; at C4 (3 slots, 32 leaves) a workgroup is
// 22 192 B, five per CU as the registers allow.
constexpr int kF4Waves = 4;
__host__ __device__ inline size_t f4_wave_bytes(int n_slots, int nl) {
  return (size_t)(n_slots > 1 ? n_slots : 1) * 4 * kWave * 4 + (size_t)nl * kWave;
}
__device__ inline float* f4_wave_lds(float* lds, int wave, int n_slots, int nl) {
  return lds + tab_floats(3) + wave * (f4_wave_bytes(n_slots, nl) / 4);
}
inline size_t f4_lds_bytes(int n_slots, int nl) {
  return (size_t)tab_floats(3) * 4 + kF4Waves * f4_wave_bytes(n_slots, nl);
}
// Sites per lane.  Only one was ever built (two doubled the adjoint's VGPRs
// and were slower at every grid measured) and the code
// carries no second one.  The one-trip `for (s < kSites)` loops that remain in
// sankoff_body, and a few copies through a local array (r, mv, buf), are there
// for the compiler alone: each leaves blocks behind that decide block order,
// the grouping of the scalar step-word loads and register numbering, and
// without any one of them the forward-bearing or Q = 3 kernels come out as
// other machine code than the one every figure in PERFLOG.md was measured on
// (PERFLOG.md, "sites-per-lane axis" section, has the experiment).  Drop them
// only together with an A/B of all 36 kernels.
constexpr int kSites = 1;
constexpr int kPrefetchRows = 64;  // leaf tiles of <= 64 leaves are prefetched

// Persistent waves: the grid holds as many waves as are co-resident; block
// (x = blockIdx % 8, j = blockIdx / 8) walks the items of XCD x's contiguous
// range with stride gridDim/8, so the waves of one XCD always work on
// adjacent tiles (shared L2 lines).  Each item is one (tree, 64-site tile);
// the next item's leaf tile is loaded into registers while the current one
// computes.
// (An LDS-resident fused variant -- every internal D vector of the tree kept
// in LDS, no adjoint re-read, one wave per SIMD -- measured 2.3x slower on the
// C4 shard and on par for C2; removed in round 3 with the other A/B-only
// variants)
//
// MULTI (sankoff_fused4.hip, not persistent): the caller is one wave of a
// multi-wave workgroup and passes its item (-1: none) and its own slot stack
// and leaf tile (wave_lds); the tables at lds are the workgroup's, written by
// every wave with the same values.  The barriers below are then the
// workgroup's: a wave without an item passes them and leaves.
template <int Q, int MODE, int PHASE, bool RAGGED, bool SYM = false, bool MULTI = false>
__device__ __forceinline__ void sankoff_body(const KArgs& A, float* lds, int wave_item = -1,
                                             float* wave_lds = nullptr) {
  constexpr bool SOFT = MODE != kHard;
  constexpr bool FWD = (PHASE & 1) != 0;
  constexpr bool BWD = (PHASE & 2) != 0;
  const int lane = MULTI ? threadIdx.x & (kWave - 1) : threadIdx.x;
  const int L = A.L;
  const float a = A.a, bcoef = A.bcoef;
  const int nb = A.nblocks;
  const int per = (nb + 7) / 8;
  const int xcd = blockIdx.x & 7;
  const int stride = gridDim.x >> 3;
  const int item_end = min(nb, (xcd + 1) * per);
  int item = xcd * per + (blockIdx.x >> 3);
  if constexpr (MULTI) {
    static_assert(PHASE != 1, "the persistent loop walks one-wave grids");
    item = wave_item;
    if (item < 0) {
      if constexpr (kPairTables) __syncthreads();
      __syncthreads();
      return;
    }
  } else {
    if (item >= item_end) return;
  }

  Coef<Q> cf;
  load_coef<Q, MODE>(A.cost, a, cf);

  float* tab = lds;
  float* slots = MULTI ? wave_lds : lds + tab_floats(PHASE);
  // pair tables (see the LDS map)
  float* tm = tab + (PHASE == 1 ? kPairFwd : kLeafTabFloats);
  float* tu = tab + kLeafTabFloats + kPairFloats;
  float* tr = tab + kLeafTabFloats + 2 * kPairFloats;
  constexpr bool PAIR_ADJ = kPairTables && BWD && MODE == kSoftK;
  constexpr int kRootSlot = 0;
  int8_t* lleaf = reinterpret_cast<int8_t*>(slots + (size_t)max(A.n_slots, 1) * Q * kWave);

  // ---- once per wave: the leaf tables.  Lane c <= Q builds row c from the
  // child row D = (0 at c, 1e5 elsewhere; all 1e5 for c = Q).  When the 1e5
  // sentinel dominates (hard: range(C) < 1e5; soft: exp(-(1e5 - range)/tau)
  // < 2^-64) a present leaf's message is exactly C[i][c] and its weights are
  // one-hot at j = c (x 1/K_ic in the factored form); otherwise (and for the
  // all-1e5 row) the tables hold the general message / weights of that row,
  // i.e. what the per-site code computes for it ----
  {
    float cmn, cmx;
    cost_range<Q>(A.cost, cmn, cmx);
    const float range = cmx - cmn;
    const bool lfast = (MODE != kHard) ? ((kSentinel - range) * a >= 64.0f) : (range < 99000.0f);
    if (lane <= Q) {
      const cptr<float> cost = as_const(A.cost);
      float d1[Q], m1[Q], g1[Q], w1[Q][Q], gc1[Q];
#pragma unroll
      for (int j = 0; j < Q; ++j) {
        d1[j] = j == lane ? 0.0f : kSentinel;
        g1[j] = 1.0f;
      }
#pragma unroll
      for (int i = 0; i < Q; ++i)
#pragma unroll
        for (int j = 0; j < Q; ++j) w1[i][j] = 0.0f;
      if (lfast && lane < Q) {
#pragma unroll
        for (int i = 0; i < Q; ++i) {
          const float cv = cost[i * Q + lane];
          m1[i] = cv;
          const float ik = MODE == kSoftK ? fast_exp2((cv - cf.cmin) * a) : 1.0f;
#pragma unroll
          for (int j = 0; j < Q; ++j) w1[i][j] = j == lane ? ik : 0.0f;
        }
      } else {
        message<Q, MODE>(cf, a, bcoef, d1, m1);
        if constexpr (BWD) message_adjoint<Q, MODE>(cf, a, d1, g1, w1, gc1);
      }
#pragma unroll
      for (int i = 0; i < Q; ++i) {
        tab[lane * Q + i] = m1[i];
        if constexpr (BWD) {  // the forward-only kernel has no W (TM lies there)
#pragma unroll
          for (int j = 0; j < Q; ++j) tab[kWTab + (lane * Q + i) * Q + j] = w1[i][j];
        }
      }
    }
  }
  // ---- once per wave: the pair tables.  Lane p < (Q + 1)^2 builds entry
  // p = c0 (Q + 1) + c1 from D = T[c0] + T[c1] (the forward's order) with the
  // per-site helpers ----
  if constexpr (kPairTables) {
    __syncthreads();  // T is written by lanes <= Q
    if (lane < (Q + 1) * (Q + 1)) {
      const int c0 = lane / (Q + 1), c1 = lane - c0 * (Q + 1);
      float t0[Q], t1[Q], d1[Q];
      lds_vec_get<Q>(tab + c0 * Q, t0);
      lds_vec_get<Q>(tab + c1 * Q, t1);
#pragma unroll
      for (int j = 0; j < Q; ++j) d1[j] = t0[j] + t1[j];
      if constexpr (FWD) {
        float m1[Q], mv[Q];
        message<Q, MODE, false>(cf, a, bcoef, d1, m1);
#pragma unroll
        for (int i = 0; i < Q; ++i) mv[i] = m1[i];
        lds_vec_put<Q>(tm + lane * Q, mv);
      }
      if constexpr (PAIR_ADJ) {
        float u[Q], rs[Q];
        softk_weights<Q, SYM>(cf, a, d1, u, rs);
        lds_vec_put<Q>(tu + lane * Q, u);
        lds_vec_put<Q>(tr + lane * Q, rs);
      }
    }
  }

  // leaf-tile prefetch: lane l loads dword (l & 15) of rows 4r + (l >> 4),
  // i.e. 16 loads cover 64 leaf rows of a 64-site tile (4-byte aligned rows)
  // (all 16 loads in flight together: one HBM round trip per tile, where the
  // byte-per-lane path waits once per batch of 8 rows).  Only the forward
  // kernel loops over items and so prefetches the NEXT tile: the adjoint's
  // register footprint is too large to keep a second tile in flight
  constexpr bool PERSIST = PHASE == 1;
  const bool pf = !RAGGED && (L & 3) == 0 && A.nl <= kPrefetchRows;
  const int pf_voff = (lane >> 4) * L + (lane & 15) * 4;
  uint32_t pre[kPrefetchRows / 4];
  auto issue_prefetch = [&](int it) {
    const int tr = it / A.tiles;
    const int tl = it - tr * A.tiles;
    const rsrc_t rl = make_rsrc(A.leaves + (size_t)tr * A.nl * L, (uint32_t)((size_t)A.nl * L));
#pragma unroll
    for (int r = 0; r < kPrefetchRows / 4; ++r)
      pre[r] = __builtin_amdgcn_raw_buffer_load_b32(rl, pf_voff, 4 * r * L + tl * kWave, kAuxLeaf);
  };
  auto store_prefetch = [&]() {
    uint32_t* dst = reinterpret_cast<uint32_t*>(lleaf);
#pragma unroll
    for (int r = 0; r < kPrefetchRows / 4; ++r) {
      const int row = 4 * r + (lane >> 4);
      if (row < A.nl) dst[row * 16 + (lane & 15)] = pre[r];
    }
  };
  if (pf) issue_prefetch(item);
  __syncthreads();  // the tables are written by lanes <= Q, read by all

  do {
    // ---- this item's tree: shape and base offsets ----
    int tree, tile, n_int, nl, Lt;
    size_t leaf_base, rows_base, site_base;  // bytes / row-sites / sites
    cptr<int> prog;
    if constexpr (RAGGED) {
      tree = as_const(A.ritem)[item];
      const cptr<int> m = as_const(A.rmeta) + (size_t)tree * kRaggedMeta;
      n_int = m[1];
      nl = m[2];
      Lt = m[3];
      site_base = (size_t)(uint32_t)m[4];
      tile = item - m[5];
      leaf_base = (size_t)(uint32_t)m[6] | ((size_t)(uint32_t)m[7] << 32);
      rows_base = (size_t)(uint32_t)m[8] | ((size_t)(uint32_t)m[9] << 32);
      prog = as_const(reinterpret_cast<const int*>(A.steps)) + (size_t)m[0] * 4;
    } else {
      tree = item / A.tiles;
      tile = item - tree * A.tiles;
      n_int = A.n_int;
      nl = A.nl;
      Lt = L;
      leaf_base = (size_t)tree * A.nl * L;
      rows_base = (size_t)tree * A.n_int * L;
      site_base = (size_t)tree * L;
      prog = as_const(reinterpret_cast<const int*>(A.steps)) + (size_t)tree * A.n_int * 4;
    }
    const int site = tile * kWave + lane;
    const bool active = site < Lt;
    const int sc = active ? site : 0;

    // ---- leaf tile of this item ----
    if (pf) {
      store_prefetch();
      if (PERSIST && item + stride < item_end) issue_prefetch(item + stride);
    } else {
      const int8_t* lv = A.leaves + leaf_base + sc;
      constexpr int kBatch = 8;
      for (int c0 = 0; c0 < nl; c0 += kBatch) {
        int code[kBatch];
        const int nb_ = min(kBatch, nl - c0);
#pragma unroll
        for (int u = 0; u < kBatch; ++u)
          if (u < nb_) code[u] = ld_code(lv + (size_t)(c0 + u) * Lt);
#pragma unroll
        for (int u = 0; u < kBatch; ++u)
          if (u < nb_) st_code(lleaf + ((c0 + u) * kWave + lane), code[u]);
      }
    }

    const uint32_t treebytes = (uint32_t)((size_t)n_int * Q * Lt * 4);
    const rsrc_t rdp = make_rsrc(A.dp + rows_base * Q, treebytes);
    // inactive lanes address past the buffer: stores drop, loads return 0
    const int voff = active ? site * Q * 4 : 0x7FFFFFF0;
    const int rowbytes = Lt * Q * 4;

    // a child's leaf code normalised to [0, Q] (Q: missing leaf / the all-1e5
    // row): leaf_code of a leaf child, child_code of a leaf or sentinel child
    auto leaf_code = [&](int desc, int& code) {
      code = ld_code(lleaf + ((desc & 0xFFFF) * kWave + lane));
      code = ((unsigned)code < (unsigned)Q) ? code : Q;
    };
    auto child_code = [&](int desc, int kind) {
      int code;
      if (kind == kKindLeaf) {
        leaf_code(desc, code);
      } else {
#pragma unroll
        for (int s = 0; s < kSites; ++s) code = Q;
      }
      return code;
    };

    float dv[Q];
    if constexpr (FWD) {
      float prev[Q];  // previous step's D (register bypass, kChildPrev)
      I4 nxt = load_step(prog, 0);
      for (int k = 0; k < n_int; ++k) {
        const I4 stp = nxt;
        if (k + 1 < n_int) nxt = load_step(prog, k + 1);
        // gather both children (LDS reads in flight together)
        float d[2][Q];
        int pair;  // c0 (Q + 1) + c1 of a step whose children are both codes
#pragma unroll
        for (int s = 0; s < kSites; ++s) pair = 0;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int desc = c == 0 ? stp.y : stp.z;
          const int kind = (desc >> 24) & 3;
          if (desc & kChildPrev) {
#pragma unroll
            for (int j = 0; j < Q; ++j)
#pragma unroll
              for (int s = 0; s < kSites; ++s) d[c][j] = prev[j];
          } else if (kind == kKindInt) {
            lds_get<Q>(slots, (desc >> 16) & 0xFF, lane, d[c]);
          } else {
            int code;  // child_code(desc, kind), spelled out (see kSites)
            if (kind == kKindLeaf) {
              leaf_code(desc, code);
            } else {
#pragma unroll
              for (int s = 0; s < kSites; ++s) code = Q;
            }
#pragma unroll
            for (int s = 0; s < kSites; ++s) {
              float r[Q];
              lds_vec_get<Q>(tab + code * Q, r);
#pragma unroll
              for (int i = 0; i < Q; ++i) d[c][i] = r[i];  // already the message
              if constexpr (kPairTables) pair = c == 0 ? code * (Q + 1) : pair + code;
            }
          }
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int desc = c == 0 ? stp.y : stp.z;
          float m[Q];
          // a deferred cherry handed its message on (TM), not its D
          if (((desc >> 24) & 3) != kKindInt || (kPairTables && (desc & kChildDeferred))) {
#pragma unroll
            for (int i = 0; i < Q; ++i)
#pragma unroll
              for (int s = 0; s < kSites; ++s) m[i] = d[c][i];
          } else {
            // the forward keeps the pair-wise dots in every kernel: the DP
            // table is bitwise the same from the fused, forward-only and
            // ragged launches (the symmetric-K form sums in another order)
            message<Q, MODE, false>(cf, a, bcoef, d[c], m);
          }
#pragma unroll
          for (int i = 0; i < Q; ++i)
#pragma unroll
            for (int s = 0; s < kSites; ++s) dv[i] = (c == 0) ? m[i] : dv[i] + m[i];
        }
        const int row = stp.x & 0xFFFF;
        const int oslot = (stp.x >> 16) & 0xFF;
        // rows the adjoint never re-reads (deferred cherries) stream past the
        // caches (nt), so the re-read rows keep more of L2 / MALL: the
        // 128-tree shard 134 -> 128 us, the full batch unchanged (its table
        // is ~10x the MALL)
        if (BWD && (stp.w & kStepDeferredIn))
          bst_row<Q, kAuxCherryRow>(rdp, voff, row * rowbytes, dv);
        else
          bst_row<Q, BWD ? kAuxFusedRow : kAuxFwdRow>(rdp, voff, row * rowbytes, dv);
        // the row is stored; its one parent takes the message from the table
        if (kPairTables && (stp.w & kStepDeferredIn)) {
#pragma unroll
          for (int s = 0; s < kSites; ++s) {
            float r[Q];
            lds_vec_get<Q>(tm + pair * Q, r);
#pragma unroll
            for (int i = 0; i < Q; ++i) dv[i] = r[i];
          }
        }
        if (!(stp.w & kStepToNext) && oslot != 0xFF) lds_put<Q>(slots, oslot, lane, dv);
#pragma unroll
        for (int i = 0; i < Q; ++i)
#pragma unroll
          for (int s = 0; s < kSites; ++s) prev[i] = dv[i];
      }
    } else {
      // adjoint only: the root row comes from the table
      bld_row<Q>(rdp, voff, (n_int - 1) * rowbytes, dv);
    }

    // ---- root: score + cotangent ----
    float score, groot[Q];
    root_score<Q, SOFT>(dv, a, bcoef, A.hard_root != 0, score, groot);
    if constexpr (FWD) {
      double tot = 0.0;
      if (active) {
#pragma unroll
        for (int s = 0; s < kSites; ++s) tot += (double)score;
        if (A.site_score) A.site_score[site_base + site] = score;
      }
      tot = wave_sum_lane0(tot);
      if (lane == 0) A.part_tree[item] = tot;
    }

    if constexpr (BWD) {
      // acc: dC accumulators (in the factored form x K[i][j] at the end; leaf
      // one-hot contributions are pre-divided by K via the IK table)
      float acc[Q][Q];
      const float dscale = A.dts ? as_const(A.dts)[tree] : 1.0f;
      const float f = active ? dscale : 0.0f;
#pragma unroll
      for (int i = 0; i < Q; ++i)
#pragma unroll
        for (int s = 0; s < kSites; ++s) groot[i] *= f;
#pragma unroll
      for (int i = 0; i < Q; ++i)
#pragma unroll
        for (int j = 0; j < Q; ++j) acc[i][j] = 0.0f;
      const bool want_marg = A.marg != nullptr;
      const rsrc_t rmg = make_rsrc(want_marg ? A.marg + rows_base * Q : A.dp, treebytes);
      int8_t* at = A.anc ? A.anc + rows_base + sc : nullptr;
      lds_put<Q>(slots, kRootSlot, lane, groot);

      // DP rows of a step's internal children are loaded one step ahead into
      // the other half of a ping-pong buffer (the loop is unrolled by two so
      // the prefetched registers are consumed in place, never copied -- a
      // copy would force a vmcnt(0) wait at the back edge).  The loads are
      // unconditional (non-internal children read past the buffer: no
      // memory traffic, zeros) so every path issues the same number of VMEM
      // ops and the compiler's vmcnt waits stay partial.
      auto prefetch = [&](const I4& s2, float (&nd)[2][Q]) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int desc = c == 0 ? s2.y : s2.z;
          // deferred cherries (kChildDeferred) are recomputed, not re-read
          const bool internal =
              ((desc >> 24) & 3) == kKindInt && !(desc & kChildDeferred);
          const int vo = internal ? voff : 0x7FFFFFF0;
          const int crow = internal ? (desc & 0xFFFF) : 0;
          bld_row<Q, FWD ? kAuxFusedLoad : kAuxAdjRow>(rdp, vo, crow * rowbytes, nd[c]);
        }
      };
      float gnext[Q];  // cotangent handed to the next reverse step (bypass)
      auto bstep = [&](const I4& stp, float (&cd)[2][Q]) {
        if (stp.w & kStepUnreached) return;
        const int row = stp.x & 0xFFFF;
        float g[Q];
        if (stp.w & kStepToNext) {
#pragma unroll
          for (int i = 0; i < Q; ++i) g[i] = gnext[i];
        } else {
          lds_get<Q>(slots, (stp.w & kStepRoot) ? kRootSlot : ((stp.x >> 16) & 0xFF), lane, g);
        }
        if (stp.w & kStepDeferredIn) {
          // g is the parent's cotangent: this step runs the parent -> cherry
          // edge adjoint the parent's step skipped
          float gc[Q];
          if constexpr (PAIR_ADJ) {
            // the edge's u and 1 / s depend on the two leaf codes only
            int pair;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
              const int desc = c == 0 ? stp.y : stp.z;
              const int code = child_code(desc, (desc >> 24) & 3);
              pair = c == 0 ? code * (Q + 1) : pair + code;
            }
            float u[Q], rs[Q];
            lds_vec_get<Q>(tu + pair * Q, u);
            lds_vec_get<Q>(tr + pair * Q, rs);
            softk_edge<Q>(cf, u, rs, g, acc, gc);
          } else {
            // the cherry's D is the sum of its two leaf messages (the
            // forward's order, so bit-identical)
            float dc[Q];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
              const int desc = c == 0 ? stp.y : stp.z;
              const int code = child_code(desc, (desc >> 24) & 3);
              float r[Q];
              lds_vec_get<Q>(tab + code * Q, r);
#pragma unroll
              for (int i = 0; i < Q; ++i) dc[i] = (c == 0) ? r[i] : dc[i] + r[i];
            }
            message_adjoint<Q, MODE, SYM>(cf, a, dc, g, acc, gc);
          }
#pragma unroll
          for (int i = 0; i < Q; ++i) g[i] = gc[i];
        }
        if (want_marg) {
          bst_row<Q, kAuxMarg>(rmg, voff, row * rowbytes, g);
        }
        if (at && active) {
          float bv = g[0];
          int bi = 0;
#pragma unroll
          for (int i = 1; i < Q; ++i)
            if (g[i] > bv) { bv = g[i]; bi = i; }
          st_code(at + (size_t)row * Lt, bi);
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int desc = c == 0 ? stp.y : stp.z;
          const int kind = (desc >> 24) & 3;
          if (kind != kKindInt) {
            // leaf / sentinel child: acc_ij += g_i W[code][i][j] (no cotangent)
            const int code = child_code(desc, kind);
#pragma unroll
            for (int s = 0; s < kSites; ++s) {
              float w[Q * Q];
              lds_vec_get<Q * Q>(tab + kWTab + code * Q * Q, w);
#pragma unroll
              for (int i = 0; i < Q; ++i) {
                float wr[Q];
#pragma unroll
                for (int j = 0; j < Q; ++j) wr[j] = w[i * Q + j];
                axpy<Q>(acc[i], g[i], wr);
              }
            }
          } else {
            float gc[Q];
            if (desc & kChildDeferred) {
              // the child's step runs this edge (kStepDeferredIn)
#pragma unroll
              for (int j = 0; j < Q; ++j) gc[j] = g[j];
            } else {
              message_adjoint<Q, MODE, SYM>(cf, a, cd[c], g, acc, gc);
            }
            if (desc & kChildPrev) {
#pragma unroll
              for (int j = 0; j < Q; ++j) gnext[j] = gc[j];
            } else if (kind == kKindInt) {
              const int cslot = (desc >> 16) & 0xFF;
              if (desc & kStepAccumulate) {
                float old[Q];
                lds_get<Q>(slots, cslot, lane, old);
#pragma unroll
                for (int j = 0; j < Q; ++j) gc[j] += old[j];
              }
              lds_put<Q>(slots, cslot, lane, gc);
            }
          }
        }
      };
      {
      // ring of kRing row buffers: step k's rows were issued kRing - 1 steps
      // earlier (more bytes in flight per wave than a ping-pong; the ring is
      // unrolled so every buffer index is static)
      constexpr int kRing = kAdjRing;
      float buf[kRing][2][Q];
      I4 sd[kRing];
      const I4 none = {0, 0, 0, 0};  // sentinel children only: prefetch reads nothing
#pragma unroll
      for (int r = 0; r < kRing - 1; ++r) {
        sd[r] = n_int - 1 - r >= 0 ? load_step(prog, n_int - 1 - r) : none;
        prefetch(sd[r], buf[r]);
      }
      I4 nd = n_int - kRing >= 0 ? load_step(prog, n_int - kRing) : none;
      for (int k = n_int - 1; k >= 0; k -= kRing) {
#pragma unroll
        for (int r = 0; r < kRing; ++r) {
          // step k - r uses buf[r]; its freed predecessor slot takes the rows
          // of step k - r - (kRing - 1) (descriptor loaded one round ahead)
          const int w = (r + kRing - 1) % kRing;
          const int j = k - r - (kRing - 1);
          sd[w] = nd;
          prefetch(sd[w], buf[w]);
          nd = j - 1 >= 0 ? load_step(prog, j - 1) : none;
          if (k - r < 0) break;
          bstep(sd[r], buf[r]);
        }
      }
      }

      // ---- per-item dC partial (fixed-order reduce kernel sums the items) ----
      if constexpr (Q == 4) {
        double v16[16];
#pragma unroll
        for (int i = 0; i < Q; ++i)
#pragma unroll
          for (int j = 0; j < Q; ++j) {
            v16[i * Q + j] = (double)acc[i][j];
            if constexpr (MODE == kSoftK) v16[i * Q + j] *= (double)cf.k[i][j];
          }
        const double v = wave_reduce_scatter16(v16, lane);
        if ((lane & 3) == 0) A.part_dc[(size_t)(lane >> 2) * nb + item] = v;
      } else {
#pragma unroll
        for (int i = 0; i < Q; ++i)
#pragma unroll
          for (int j = 0; j < Q; ++j) {
            double v = (double)acc[i][j];
            if constexpr (MODE == kSoftK) v = v * (double)cf.k[i][j];
            v = wave_sum_lane0(v);
            if (lane == 0) A.part_dc[(size_t)(i * Q + j) * nb + item] = v;
          }
      }
    }
    item += stride;
  } while (PERSIST && item < item_end);
}

}  // namespace

}  // namespace trex
