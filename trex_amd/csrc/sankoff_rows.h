// Lane-per-site row passes on the Sankoff DP table: what every pass shares (the
// argument record PassArgs, the variant dispatcher with_variant, the entry
// points' body run_pass, the shape and workspace arithmetic, the row helpers)
// and the kernels that both leaf types use: the pre-order
// "outside" pass, the O(Q^2) evaluation of every nearest-neighbour interchange
// per site (DESIGN.md "NNI neighbour scoring") and the attachment scores.
// Included by sankoff_nni.hip (int8 codes), sankoff_sets.hip (int32 state
// sets, DESIGN.md "State-set leaves"; it adds the state-set forward) and
// sankoff_spr.hip (the SPR kernel, both leaf types).  The leaf type LT is a
// template parameter that reaches exactly one place, leaf_row: everything
// else is one copy of the arithmetic.
//
// One tree, one site; (+) is min for tau = 0 and smin_tau for tau > 0;
// C[parent][child]; D_x is node x's inside row (leaf: 0 at its code / at the
// set bits of its mask, 1e5 elsewhere; internal: the DP-table row):
//   message       M_x[i] = (+)_j (C[i][j] + D_x[j])
//   outside row   O_root = 0;  O_c[j] = (+)_i (C[i][j] + O_p[i] + M_s[i])
//                 (p = c's parent, s = c's sibling)
//   move (v, k)   swaps a_k of (a0, a1) = children[v] with v's sibling s
//                 (u = v's parent):  D'_v = M_s + M_a(1-k),
//                 site score = (+)_i (O_u[i] + M_ak[i] + M(D'_v)[i])
// Every kernel gives one 64-lane wave 64 consecutive sites of ONE tree (sites
// on the lane axis), so the plan words (plan.cpp, NNI / attach plan) and the
// cost matrix are wave-uniform and read with scalar loads.  Q = 2, 3, 4 are
// compile-time instantiations with every row in registers and one 8 / 12 /
// 16-byte buffer access per row and lane; 4 < Q <= 20 runs the same code
// padded to 20 states with wave-uniform guards on the live ones.  The softmin
// is the stabilised form (row minimum subtracted).  Scores are summed over a
// wave's sites in fp64 (fixed butterfly), the per-wave partials over a tree's
// tiles in a fixed order by a second kernel: no float atomics, bitwise
// reproducible.  With site weights (DESIGN.md "Site weights") a site's score
// is multiplied by its weight in fp64 where it enters that sum and nowhere
// else; the WT = false instantiations are the unweighted code.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "sankoff_dev.h"
#include "trex_common.h"

namespace trex {

namespace {

constexpr int kRowsPadQ = kSiteMaxQ;  // the generic path's padded alphabet

// ---- shapes: one wave per 64-site tile of one tree; a pass scores `moves`
// entries per tree and its waves write [B * tiles][moves] fp64 partials.  The
// *_workspace_bytes functions and the reduce take the counts from here; a
// kernel's `part` offset is blockIdx.x times the same product, spelled out.
constexpr int tiles(int L) { return (L + kWave - 1) / kWave; }
inline int nni_moves(int n_all) { return (tree_ni(n_all) - 1) * 2; }
inline int attach_moves(int n_all) { return n_all; }
inline int64_t spr_moves(int n_all) { return (int64_t)(n_all - 1) * n_all; }

// the shapes for which the *_workspace_bytes functions answer (0 otherwise)
inline bool workspace_shape_ok(int B, int L, int n_all, int Q) {
  return !(B <= 0 || L <= 0 || n_all < 5 || n_all % 2 == 0 || Q < 2 || Q > kSiteMaxQ);
}
inline int64_t partials_workspace_bytes(int B, int L, int n_all, int Q, int64_t moves) {
  if (!workspace_shape_ok(B, L, n_all, Q)) return 0;
  return (int64_t)B * tiles(L) * moves * 8 + 256;
}

// The argument record of every pass.  plan: the pass's plan, its per-tree
// regions (past the header); part: the pass's [B * tiles][moves] partials.
// What only one pass takes rides behind it (AttachArgs, SprArgs, SetsFwdArgs).
template <class LT>
struct PassArgs {
  const int* plan;
  const LT* leaves;
  const float* cost;
  const float* dp;
  float* outside;  // null in the state-set forward, which has none (SetsFwdArgs)
  double* part;
  int B, L, nl, ni, Q, tiles;
  float a, bcoef;
};

// DYN = false: Q == QP at compile time, the matrix in SGPRs.  DYN = true: QP
// padded states, the live ones are j < Q (wave-uniform), matrix entries are
// scalar loads at their use.
template <int QP, bool DYN>
struct CostM {
  float c[DYN ? 1 : QP][DYN ? 1 : QP];
  cptr<float> p;
  int Q;
  __device__ __forceinline__ void load(const float* cost, int q) {
    p = as_const(cost);
    Q = q;
    if constexpr (!DYN) {
#pragma unroll
      for (int i = 0; i < QP; ++i)
#pragma unroll
        for (int j = 0; j < QP; ++j) c[i][j] = p[i * QP + j];
    }
  }
  __device__ __forceinline__ bool live(int j) const { return !DYN || j < Q; }
  __device__ __forceinline__ float at(int i, int j) const {
    if constexpr (DYN) return p[i * Q + j];
    else return c[i][j];
  }
};

// (+) over the live entries of x
template <int QP, bool DYN, bool SOFT>
__device__ __forceinline__ float oplus(const CostM<QP, DYN>& cm, float a, float bcoef,
                                       const float (&x)[QP]) {
  float mn = INFINITY;
#pragma unroll
  for (int j = 0; j < QP; ++j)
    if (cm.live(j)) mn = fminf(mn, x[j]);
  if constexpr (!SOFT) return mn;
  float acc = 0.0f;
#pragma unroll
  for (int j = 0; j < QP; ++j)
    if (cm.live(j)) acc += fast_exp2((mn - x[j]) * a);
  return fmaf(-bcoef, fast_log2(acc), mn);
}

// m[i] = (+)_j (C[i][j] + d[j]);  TRANS: m[j] = (+)_i (C[i][j] + d[i])
template <int QP, bool DYN, bool SOFT, bool TRANS = false>
__device__ __forceinline__ void message(const CostM<QP, DYN>& cm, float a, float bcoef,
                                        const float (&d)[QP], float (&m)[QP]) {
#pragma unroll
  for (int i = 0; i < QP; ++i) {
    m[i] = 0.0f;
    if (cm.live(i)) {
      float x[QP];
#pragma unroll
      for (int j = 0; j < QP; ++j) {
        x[j] = 0.0f;
        if (cm.live(j)) x[j] = (TRANS ? cm.at(j, i) : cm.at(i, j)) + d[j];
      }
      m[i] = oplus<QP, DYN, SOFT>(cm, a, bcoef, x);
    }
  }
}

// one tree's DP-layout table ([row][L][Q]): the lane's site of a row
template <int QP, bool DYN>
struct Rows {
  rsrc_t r;
  const float* base;
  int L, Q, site;
  __device__ __forceinline__ void init(const float* tree_base, int ni, int L_, int Q_, int site_) {
    base = tree_base;
    L = L_;
    Q = Q_;
    site = site_;
    if constexpr (!DYN) r = make_rsrc(tree_base, (uint32_t)((size_t)ni * L_ * QP * 4));
  }
  __device__ __forceinline__ void get(int row, float (&d)[QP]) const {
    if constexpr (!DYN) {
      bld_row<QP>(r, site * QP * 4, row * L * QP * 4, d);
    } else {
      const float* p = base + ((size_t)row * L + site) * Q;
#pragma unroll
      for (int j = 0; j < QP; ++j) d[j] = j < Q ? p[j] : 0.0f;
    }
  }
  __device__ __forceinline__ void put(int row, const float (&d)[QP]) const {
    if constexpr (!DYN) {
      bst_row<QP>(r, site * QP * 4, row * L * QP * 4, d);
    } else {
      float* p = const_cast<float*>(base) + ((size_t)row * L + site) * Q;
#pragma unroll
      for (int j = 0; j < QP; ++j)
        if (j < Q) p[j] = d[j];
    }
  }
};

// A leaf's inside row from its cell: an int8 code (0 at the code; -1 and any
// other code out of range: all 1e5) or an int32 state set (0 where bit j is
// set).  Only j < QP is looked at and the padded path reads only its live
// j < Q, so a mask's bits at or above Q never matter.
template <int QP>
__device__ __forceinline__ void leaf_row(int8_t cell, float (&d)[QP]) {
  const int code = cell;
#pragma unroll
  for (int j = 0; j < QP; ++j) d[j] = code == j ? 0.0f : kSentinel;
}
template <int QP>
__device__ __forceinline__ void leaf_row(int32_t mask, float (&d)[QP]) {
#pragma unroll
  for (int j = 0; j < QP; ++j) d[j] = (mask >> j) & 1 ? 0.0f : kSentinel;
}

// inside row of a plan descriptor (kind << 24 | index): a leaf's row from its
// cell, an internal node's from the DP table
template <int QP, bool DYN, class LT>
__device__ __forceinline__ void inside_row(int desc, const Rows<QP, DYN>& dp,
                                           const LT* __restrict__ tree_leaves, int L, int site,
                                           float (&d)[QP]) {
  const int idx = desc & 0xFFFF;
  if ((desc >> 24) == kKindLeaf) {
    leaf_row<QP>(tree_leaves[(size_t)idx * L + site], d);
  } else {
    dp.get(idx, d);
  }
}

// The lane's site weight as the fp64 factor of its site scores: one coalesced
// 256-byte read per wave at the clamped site.  A tail lane holds the last
// site's weight and is masked by a select where the sums are taken, so it adds
// nothing whatever that weight is.  Unweighted: exactly 1.0 (x * 1.0 is exact).
// The weights ([B][L], or null) are a kernel argument of their own behind the
// argument record, so the WT = false kernels read the record they always read.
template <bool WT>
__device__ __forceinline__ double site_weight(const float* weights, int b, int L, int site) {
  if constexpr (WT) return (double)weights[(size_t)b * L + site];
  else return 1.0;
}

// The tail-lane rule of every kernel of this family: a lane past the last site
// (!on) recomputes the last site (`site` is clamped), stores no row and no
// site score, and is masked out of the wave sums by a select.
//
// Outside pass: a wave walks its tree's internal nodes in pre-order, reading
// the parent's outside row it wrote earlier (same lane, same address) and the
// sibling's inside row, writing the node's outside row.
template <class LT, int QP, bool DYN, bool SOFT>
__global__ __launch_bounds__(kWave) void outside_kernel(const PassArgs<LT> A) {
  const int lane = threadIdx.x;
  const int b = blockIdx.x / A.tiles, tile = blockIdx.x % A.tiles;
  const int l = tile * kWave + lane;
  const bool on = l < A.L;
  const int site = on ? l : A.L - 1;  // tail lanes recompute the last site, store nothing
  CostM<QP, DYN> cm;
  cm.load(A.cost, A.Q);
  const size_t tree = (size_t)b * A.ni * A.L * A.Q;
  Rows<QP, DYN> dp, out;
  dp.init(A.dp + tree, A.ni, A.L, A.Q, site);
  out.init(A.outside + tree, A.ni, A.L, A.Q, site);
  const LT* lv = A.leaves + (size_t)b * A.nl * A.L;
  const cptr<int> pre = as_const(A.plan) + (size_t)b * (8 * A.ni - 4);
  for (int k = 0; k < A.ni; ++k) {
    const I4 e = load_step(pre, k);
    float oc[QP];
    if (e.y < 0) {
#pragma unroll
      for (int j = 0; j < QP; ++j) oc[j] = 0.0f;
    } else {
      float t[QP], ds[QP], ms[QP];
      out.get(e.y, t);
      inside_row<QP, DYN>(e.z, dp, lv, A.L, site, ds);
      message<QP, DYN, SOFT>(cm, A.a, A.bcoef, ds, ms);
#pragma unroll
      for (int i = 0; i < QP; ++i) t[i] += ms[i];
      message<QP, DYN, SOFT, true>(cm, A.a, A.bcoef, t, oc);
    }
    if (on) out.put(e.x, oc);
  }
}

// Neighbour scores: per non-root internal v both moves' site scores, summed
// over the wave's sites in fp64; lane 0 writes the two partials.
template <class LT, int QP, bool DYN, bool SOFT, bool WT>
__global__ __launch_bounds__(kWave) void nni_score_kernel(const PassArgs<LT> A,
                                                          const float* weights) {
  const int lane = threadIdx.x;
  const int b = blockIdx.x / A.tiles, tile = blockIdx.x % A.tiles;
  const int l = tile * kWave + lane;
  const bool on = l < A.L;
  const int site = on ? l : A.L - 1;
  const double w = site_weight<WT>(weights, b, A.L, site);
  CostM<QP, DYN> cm;
  cm.load(A.cost, A.Q);
  const size_t tree = (size_t)b * A.ni * A.L * A.Q;
  Rows<QP, DYN> dp, out;
  dp.init(A.dp + tree, A.ni, A.L, A.Q, site);
  out.init(A.outside + tree, A.ni, A.L, A.Q, site);
  const LT* lv = A.leaves + (size_t)b * A.nl * A.L;
  const cptr<int> mv = as_const(A.plan) + (size_t)b * (8 * A.ni - 4) + 4 * A.ni;
  double* part = A.part + (size_t)blockIdx.x * (A.ni - 1) * 2;
  for (int e = 0; e < A.ni - 1; ++e) {
    const I4 m = load_step(mv, e);
    float ou[QP], d[QP], m0[QP], m1[QP], ms[QP];
    out.get(m.x, ou);
    inside_row<QP, DYN>(m.y, dp, lv, A.L, site, d);
    message<QP, DYN, SOFT>(cm, A.a, A.bcoef, d, m0);
    inside_row<QP, DYN>(m.z, dp, lv, A.L, site, d);
    message<QP, DYN, SOFT>(cm, A.a, A.bcoef, d, m1);
    inside_row<QP, DYN>(m.w, dp, lv, A.L, site, d);
    message<QP, DYN, SOFT>(cm, A.a, A.bcoef, d, ms);
    float sc[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      // v keeps a(1-k) and takes s; u keeps v and takes ak
      float dv[QP], mdv[QP], x[QP];
#pragma unroll
      for (int j = 0; j < QP; ++j) dv[j] = ms[j] + (k == 0 ? m1[j] : m0[j]);
      message<QP, DYN, SOFT>(cm, A.a, A.bcoef, dv, mdv);
#pragma unroll
      for (int i = 0; i < QP; ++i) x[i] = ou[i] + (k == 0 ? m0[i] : m1[i]) + mdv[i];
      sc[k] = oplus<QP, DYN, SOFT>(cm, A.a, A.bcoef, x);
    }
    const double s0 = wave_sum_lane0(on ? (double)sc[0] * w : 0.0);
    const double s1 = wave_sum_lane0(on ? (double)sc[1] * w : 0.0);
    if (lane == 0) {
      part[2 * e] = s0;
      part[2 * e + 1] = s1;
    }
  }
}

// score[b][e][k] = the tiles' partials summed in tile order, rounded to fp32
__global__ __launch_bounds__(256) void reduce_partials_kernel(const double* __restrict__ part,
                                                              int B, int tiles, int moves,
                                                              float* __restrict__ score) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)B * moves) return;
  const int64_t b = t / moves, m = t % moves;
  const double* p = part + b * tiles * moves + m;
  double acc = 0.0;
  for (int k = 0; k < tiles; ++k) acc += p[(int64_t)k * moves];
  score[t] = (float)acc;
}

// part [B][tiles][moves] -> score [B][moves] on the stream
inline void reduce_partials(hipStream_t st, const double* part, int B, int tiles, int moves,
                            float* score) {
  const int64_t n = (int64_t)B * moves;
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                     part, B, tiles, moves, score);
}

// ---- host side of every pass ----------------------------------------------
// A kernel variant as compile-time tags: Q = QP in registers or (DYN) padded to
// QP states; (+) hard or soft; site weights or none.
template <int QP_, bool SOFT_, bool WT_>
struct Variant {
  static constexpr int QP = QP_;
  static constexpr bool DYN = QP_ > 4, SOFT = SOFT_, WT = WT_;
};

// f(Variant<...>()) for the call's (Q, soft, weighted).  A pass without a
// weighted form passes weighted = false and has no WT parameter to instantiate.
template <class F>
void with_variant(int Q, bool soft, bool weighted, F&& f) {
  auto rest = [&](auto qp) {
    constexpr int QP = decltype(qp)::value;
    if (soft) {
      if (weighted) f(Variant<QP, true, true>());
      else f(Variant<QP, true, false>());
    } else {
      if (weighted) f(Variant<QP, false, true>());
      else f(Variant<QP, false, false>());
    }
  };
  switch (Q) {
    case 2: rest(std::integral_constant<int, 2>()); break;
    case 3: rest(std::integral_constant<int, 3>()); break;
    case 4: rest(std::integral_constant<int, 4>()); break;
    default: rest(std::integral_constant<int, kRowsPadQ>()); break;
  }
}

inline int pass_check_shape(const char* fn, int B, int L, int n_all, int Q, float tau) {
  if (B <= 0 || L <= 0 || n_all < 3 || n_all > 65535 || n_all % 2 == 0 || Q < 2)
    return set_error(TREX_E_ARG, "%s: bad shape B=%d L=%d n_all=%d Q=%d", fn, B, L, n_all, Q);
  if (n_all < 5)
    return set_error(TREX_E_TOPOLOGY, "%s: a tree of %d leaves has no NNI neighbours", fn,
                     (n_all + 1) / 2);
  if (Q > kSiteMaxQ)
    return set_error(TREX_E_UNSUPPORTED, "%s: Q=%d > %d is not supported by the NNI kernels", fn,
                     Q, kSiteMaxQ);
  if (!nonneg_finite_f32(tau))
    return set_error(TREX_E_ARG, "%s: tau must be finite and >= 0 (got %g)", fn, tau);
  if ((int64_t)tree_ni(n_all) * L * Q * 4 > 0x7FFFFFF0LL)
    return set_error(TREX_E_UNSUPPORTED, "%s: one tree's DP table exceeds 2 GiB", fn);
  if ((int64_t)B * tiles(L) > 0x7FFFFFFF)
    return set_error(TREX_E_ARG, "%s: grid too large", fn);
  return TREX_OK;
}

// An entry point's arguments.  A pass that lacks one leaves it null / 0:
// outside (the state-set forward), weights, score and the workspace (the
// outside pass, which sums nothing).
template <class LT>
struct PassCall {
  const char* fn;
  const int32_t* plan;
  const LT* leaves;
  const float* cost;
  int B, L, n_all, Q;
  float tau;
  const float* dp;
  float* outside;
  const float* weights;
  float* score;  // [B][moves]
  void* workspace;
  int64_t workspace_bytes;
  void* stream;
};

// The body of every entry point.  rest_given: the pass's own pointers besides
// plan / leaves / cost / dp are non-null.  pre(need): the pass's own argument
// checks, then the workspace bytes it needs.  moves: score entries per tree (0:
// no partials to sum).  launch(A, stream): the pass's kernel on the filled
// record.
template <class LT, class Pre, class Launch>
int run_pass(const PassCall<LT>& c, bool rest_given, Pre&& pre, int moves, Launch&& launch) {
  if (int e = pass_check_shape(c.fn, c.B, c.L, c.n_all, c.Q, c.tau)) return e;
  if (!c.plan || !c.leaves || !c.cost || !c.dp || !rest_given)
    return set_error(TREX_E_ARG, "%s: null pointer argument", c.fn);
  int64_t need = 0;
  if (int e = pre(need)) return e;
  if (c.workspace_bytes < need) return set_error(TREX_E_ARG, "%s: workspace too small", c.fn);
  PassArgs<LT> A;
  A.plan = c.plan + TREX_PLAN_HEADER_INTS;
  A.leaves = c.leaves;
  A.cost = c.cost;
  A.dp = c.dp;
  A.outside = c.outside;
  A.part = static_cast<double*>(c.workspace);
  A.B = c.B;
  A.L = c.L;
  A.nl = tree_nl(c.n_all);
  A.ni = tree_ni(c.n_all);
  A.Q = c.Q;
  A.tiles = tiles(c.L);
  tau_coefs(c.tau, &A.a, &A.bcoef);
  hipStream_t st = (hipStream_t)c.stream;
  launch(A, st);
  if (int e = hip_check(c.fn)) return e;
  if (moves == 0) return TREX_OK;
  reduce_partials(st, A.part, c.B, A.tiles, moves, c.score);
  return hip_check(c.fn);
}

template <class LT>
int outside_run(const PassCall<LT>& c) {
  return run_pass(
      c, c.outside != nullptr, [](int64_t&) { return TREX_OK; }, 0,
      [&](const PassArgs<LT>& A, hipStream_t st) {
        with_variant(c.Q, c.tau > 0.0f, false, [&](auto v) {
          using V = decltype(v);
          hipLaunchKernelGGL((outside_kernel<LT, V::QP, V::DYN, V::SOFT>), dim3(A.B * A.tiles),
                             dim3(kWave), 0, st, A);
        });
      });
}

template <class LT>
int nni_run(const PassCall<LT>& c) {
  return run_pass(
      c, c.outside && c.score && c.workspace,
      [&](int64_t& need) {
        need = trex_nni_workspace_bytes(c.B, c.L, c.n_all, c.Q);
        return TREX_OK;
      },
      nni_moves(c.n_all), [&](const PassArgs<LT>& A, hipStream_t st) {
        with_variant(c.Q, c.tau > 0.0f, c.weights != nullptr, [&](auto v) {
          using V = decltype(v);
          hipLaunchKernelGGL((nni_score_kernel<LT, V::QP, V::DYN, V::SOFT, V::WT>),
                             dim3(A.B * A.tiles), dim3(kWave), 0, st, A, c.weights);
        });
      });
}

// ---- attachment scores (DESIGN.md "Attachment scores") -------------------
// Attaching a subtree with inside row D_new (message M_new) on the edge above
// node x makes a new node w with children x and the subtree:
//   x below p, sibling s:  D_w = M_x + M_new,
//                          site score = (+)_i (O_p[i] + M_s[i] + M(D_w)[i])
//   x the root:            site score = (+)_k (M_root[k] + M_new[k])
template <class LT>
struct AttachArgs : PassArgs<LT> {
  const LT* sub_codes;    // [B][L] leaf cells, or
  const float* sub_rows;  // [B][L][Q]
};

__device__ __forceinline__ int desc_node(int desc, int nl) {
  return (desc >> 24) == kKindLeaf ? (desc & 0xFFFF) : nl + (desc & 0xFFFF);
}

// A wave walks its tree's internal rows p: both child edges of p from O_p and
// the children's messages, on the root row also the new-root entry; site sums
// in fp64, lane 0 writes the partials at the edges' lower node ids.
template <class LT, int QP, bool DYN, bool SOFT, bool WT>
__global__ __launch_bounds__(kWave) void attach_score_kernel(const AttachArgs<LT> AA,
                                                             const float* weights) {
  const PassArgs<LT>& A = AA;
  const int lane = threadIdx.x;
  const int b = blockIdx.x / A.tiles, tile = blockIdx.x % A.tiles;
  const int l = tile * kWave + lane;
  const bool on = l < A.L;
  const int site = on ? l : A.L - 1;
  const double w = site_weight<WT>(weights, b, A.L, site);
  CostM<QP, DYN> cm;
  cm.load(A.cost, A.Q);
  const size_t tree = (size_t)b * A.ni * A.L * A.Q;
  Rows<QP, DYN> dp, out;
  dp.init(A.dp + tree, A.ni, A.L, A.Q, site);
  out.init(A.outside + tree, A.ni, A.L, A.Q, site);
  const LT* lv = A.leaves + (size_t)b * A.nl * A.L;
  const cptr<int> pl = as_const(A.plan) + (size_t)b * 4 * A.ni;
  const int n_all = A.nl + A.ni;
  double* part = A.part + (size_t)blockIdx.x * n_all;
  float mn[QP];
  {
    float dn[QP];
    if (AA.sub_codes) {
      leaf_row<QP>(AA.sub_codes[(size_t)b * A.L + site], dn);
    } else {
      Rows<QP, DYN> sub;
      sub.init(AA.sub_rows + (size_t)b * A.L * A.Q, 1, A.L, A.Q, site);
      sub.get(0, dn);
    }
    message<QP, DYN, SOFT>(cm, A.a, A.bcoef, dn, mn);
  }
  for (int r = 0; r < A.ni; ++r) {
    const I4 e = load_step(pl, r);
    float op[QP], d[QP], m0[QP], m1[QP];
    out.get(e.x, op);
    inside_row<QP, DYN>(e.y, dp, lv, A.L, site, d);
    message<QP, DYN, SOFT>(cm, A.a, A.bcoef, d, m0);
    inside_row<QP, DYN>(e.z, dp, lv, A.L, site, d);
    message<QP, DYN, SOFT>(cm, A.a, A.bcoef, d, m1);
    float sc[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      // the edge above child k: w takes child k and the subtree, p keeps the other child
      float dw[QP], mdw[QP], x[QP];
#pragma unroll
      for (int j = 0; j < QP; ++j) dw[j] = (k == 0 ? m0[j] : m1[j]) + mn[j];
      message<QP, DYN, SOFT>(cm, A.a, A.bcoef, dw, mdw);
#pragma unroll
      for (int i = 0; i < QP; ++i) x[i] = op[i] + (k == 0 ? m1[i] : m0[i]) + mdw[i];
      sc[k] = oplus<QP, DYN, SOFT>(cm, A.a, A.bcoef, x);
    }
    const double s0 = wave_sum_lane0(on ? (double)sc[0] * w : 0.0);
    const double s1 = wave_sum_lane0(on ? (double)sc[1] * w : 0.0);
    if (lane == 0) {
      part[desc_node(e.y, A.nl)] = s0;
      part[desc_node(e.z, A.nl)] = s1;
    }
    if (e.w) {  // a new root above the old one
      float x[QP];
      dp.get(e.x, d);
      message<QP, DYN, SOFT>(cm, A.a, A.bcoef, d, m0);
#pragma unroll
      for (int i = 0; i < QP; ++i) x[i] = m0[i] + mn[i];
      const float sr = oplus<QP, DYN, SOFT>(cm, A.a, A.bcoef, x);
      const double s2 = wave_sum_lane0(on ? (double)sr * w : 0.0);
      if (lane == 0) part[A.nl + e.x] = s2;
    }
  }
}

// sub_name: what the entry point calls its leaf-cell subtree argument
template <class LT>
int attach_run(const PassCall<LT>& c, const char* sub_name, const LT* sub_codes,
               const float* sub_rows) {
  return run_pass(
      c, c.outside && c.score && c.workspace,
      [&](int64_t& need) {
        if ((sub_codes == nullptr) == (sub_rows == nullptr))
          return set_error(TREX_E_ARG, "%s: exactly one of %s and sub_rows must be given", c.fn,
                           sub_name);
        need = trex_attach_workspace_bytes(c.B, c.L, c.n_all, c.Q);
        return TREX_OK;
      },
      attach_moves(c.n_all), [&](const PassArgs<LT>& A, hipStream_t st) {
        const AttachArgs<LT> AA{A, sub_codes, sub_rows};
        with_variant(c.Q, c.tau > 0.0f, c.weights != nullptr, [&](auto v) {
          using V = decltype(v);
          hipLaunchKernelGGL((attach_score_kernel<LT, V::QP, V::DYN, V::SOFT, V::WT>),
                             dim3(A.B * A.tiles), dim3(kWave), 0, st, AA, c.weights);
        });
      });
}

}  // namespace

}  // namespace trex
