// Per-branch change counts and branch lengths on the Sankoff DP and outside
// tables (DESIGN.md "Per-branch changes"; definitions: include/trex_hip.h), for
// leaves given as int8 codes and as int32 state sets, over the row helpers of
// sankoff_rows.h.
//
// For the edge from parent p to child c with sibling s the joint cost of state
// i at p and state j at c is
//   J[i][j] = O_p[i] + M_s[i] + C[i][j] + D_c[j],     (+)_ij J = the site score.
// One 64-lane wave takes 64 consecutive sites of ONE tree and walks the attach
// plan's internal rows p: O_p, both children's inside rows and messages, then
// per child edge
//   tau > 0   P[i][j] = exp2((min J - J[i][j]) a) / sum: the Gibbs posterior of
//             the pair, normalised by the lane's own sum;
//   tau = 0   the pair (state_p, state_c) of the caller's reconstruction (a
//             leaf child: the first-index argmin_j of C[state_p][j] + D_c[j]),
//             and the least and the largest C[i][j] over the pairs with
//             J[i][j] == min J.
// Every entry is multiplied by the site's weight in fp64 and summed over the
// wave (fixed butterfly); the per-tile partials [B * tiles][n_all][E], E = Q^2
// (+ 2 at tau = 0: min, max), are written at the child's node id.  The root's
// slot is never written nor read.  edge_reduce_kernel sums the tiles in order
// (coalesced: one thread per entry), leaves the fp64 total in tile 0's slot and
// writes the fp32 outputs; edge_length_kernel forms lengths = sum_ij counts C
// from those fp64 totals.  No atomics: repeated calls are bitwise equal.
// Q = 2, 3, 4 hold an edge's J in registers (Q = 4: one reduce-scatter of the
// 16 sums); the padded path never does: one sweep for the minimum and the
// normaliser, then one out-of-line call per live row i that forms, sums and
// stores that row's entries.  Owns trex_edge_workspace_bytes,
// trex_sankoff_edge_changes_w and trex_sankoff_sets_edge_changes_w.
#include <climits>

#include "sankoff_rows.h"

namespace trex {

namespace {

template <class LT>
struct EdgeArgs : PassArgs<LT> {
  const int8_t* states;  // [B][ni][L], tau = 0 only
  int E;                 // entries per edge: Q^2 (+ 2 at tau = 0)
};

// message() of sankoff_rows.h, out of line on the padded path as in
// sankoff_spr.hip (one copy per SOFT instead of 20 x 20 terms per site)
template <int QP, bool SOFT>
__device__ __noinline__ void message_padded(const CostM<QP, true>& cm, float a, float bcoef,
                                            const float (&d)[QP], float (&m)[QP]) {
  message<QP, true, SOFT>(cm, a, bcoef, d, m);
}
template <int QP, bool DYN, bool SOFT>
__device__ __forceinline__ void msg(const CostM<QP, DYN>& cm, float a, float bcoef,
                                    const float (&d)[QP], float (&m)[QP]) {
  if constexpr (DYN) message_padded<QP, SOFT>(cm, a, bcoef, d, m);
  else message<QP, DYN, SOFT>(cm, a, bcoef, d, m);
}

// J[i][j]: the one spelling every sweep uses, so a recomputed J has the same bits
template <int QP, bool DYN>
__device__ __forceinline__ float joint(const CostM<QP, DYN>& cm, float base_i, int i, int j,
                                       const float (&d)[QP]) {
  return base_i + (cm.at(i, j) + d[j]);
}

// Padded path, row i of an edge: its Q entries formed, summed over the wave and
// stored by lane 0.  Soft: P[i][j] * w; hard: w_i where the child's state is j
// (w_i = the lane's weight if its parent state is i, else 0).
template <int QP, bool SOFT>
__device__ __noinline__ void edge_row_padded(const CostM<QP, true>& cm, float a, int i,
                                             float base_i, const float (&d)[QP], float mn,
                                             float inv, double w_i, int sc, double* pe_row,
                                             int lane) {
#pragma unroll
  for (int j = 0; j < QP; ++j) {
    if (!cm.live(j)) continue;
    double v;
    if constexpr (SOFT)
      v = (double)(fast_exp2((mn - joint<QP, true>(cm, base_i, i, j, d)) * a) * inv) * w_i;
    else
      v = sc == j ? w_i : 0.0;
    const double s = wave_sum_lane0(v);
    if (lane == 0) pe_row[j] = s;
  }
}

// One edge: base[i] = O_p[i] + M_s[i], d = D_c.  won: the lane's weight, 0 on a
// tail lane.  Hard: sp = the parent's state, leaf / sc_in: the child is a leaf
// (its state is the argmin) or its state from the reconstruction.
template <int QP, bool DYN, bool SOFT>
__device__ __forceinline__ void edge_sums(const CostM<QP, DYN>& cm, const float* cost, float a,
                                          const float (&base)[QP], const float (&d)[QP],
                                          double won, int sp, bool leaf, int sc_in, double* pe,
                                          int lane) {
  const int Q = DYN ? cm.Q : QP;
  float mn = INFINITY;
#pragma unroll
  for (int i = 0; i < QP; ++i)
#pragma unroll
    for (int j = 0; j < QP; ++j)
      if (cm.live(i) && cm.live(j)) mn = fminf(mn, joint<QP, DYN>(cm, base[i], i, j, d));
  float inv = 0.0f, lo = INFINITY, hi = -INFINITY;
  if constexpr (SOFT) {
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < QP; ++i)
#pragma unroll
      for (int j = 0; j < QP; ++j)
        if (cm.live(i) && cm.live(j))
          acc += fast_exp2((mn - joint<QP, DYN>(cm, base[i], i, j, d)) * a);
    inv = 1.0f / acc;
  } else {
#pragma unroll
    for (int i = 0; i < QP; ++i)
#pragma unroll
      for (int j = 0; j < QP; ++j)
        if (cm.live(i) && cm.live(j)) {
          const float c = cm.at(i, j);
          const bool tie = joint<QP, DYN>(cm, base[i], i, j, d) == mn;
          lo = tie ? fminf(lo, c) : lo;
          hi = tie ? fmaxf(hi, c) : hi;
        }
  }
  // hard: the pair of states this lane counts; ok: both are states
  bool ok = false;
  int sc = 0;
  if constexpr (!SOFT) {
    ok = sp >= 0 && sp < Q;
    if (leaf) {
      const int spc = ok ? sp : 0;
      float best = INFINITY;
#pragma unroll
      for (int j = 0; j < QP; ++j) {
        if (!cm.live(j)) continue;
        float c;
        if constexpr (DYN) {
          c = cost[spc * Q + j];
        } else {
          c = cm.c[0][j];
#pragma unroll
          for (int i = 1; i < QP; ++i) c = spc == i ? cm.c[i][j] : c;
        }
        const float x = c + d[j];
        if (x < best) {
          best = x;
          sc = j;
        }
      }
    } else {
      sc = sc_in;
      ok = ok && sc >= 0 && sc < Q;
    }
  }
  if constexpr (DYN) {
#pragma unroll
    for (int i = 0; i < QP; ++i)
      if (cm.live(i))
        edge_row_padded<QP, SOFT>(cm, a, i, base[i], d, mn, inv,
                                  SOFT ? won : (ok && sp == i ? won : 0.0), sc, pe + i * Q, lane);
  } else {
    double v[QP * QP];
#pragma unroll
    for (int i = 0; i < QP; ++i)
#pragma unroll
      for (int j = 0; j < QP; ++j) {
        if constexpr (SOFT)
          v[i * QP + j] =
              (double)(fast_exp2((mn - joint<QP, DYN>(cm, base[i], i, j, d)) * a) * inv) * won;
        else
          v[i * QP + j] = ok && sp == i && sc == j ? won : 0.0;
      }
    if constexpr (QP == 4) {
      const double x = wave_reduce_scatter16(v, lane);  // lane 4 q holds entry q
      if ((lane & 3) == 0) pe[lane >> 2] = x;
    } else {
#pragma unroll
      for (int q = 0; q < QP * QP; ++q) {
        const double s = wave_sum_lane0(v[q]);
        if (lane == 0) pe[q] = s;
      }
    }
  }
  if constexpr (!SOFT) {
    const double s0 = wave_sum_lane0((double)lo * won);
    const double s1 = wave_sum_lane0((double)hi * won);
    if (lane == 0) {
      pe[Q * Q] = s0;
      pe[Q * Q + 1] = s1;
    }
  }
}

// A wave walks its tree's internal rows p: both child edges of p, the partials
// at the edges' lower node ids.
template <class LT, int QP, bool DYN, bool SOFT, bool WT>
__global__ __launch_bounds__(kWave) void edge_changes_kernel(const EdgeArgs<LT> EA,
                                                             const float* weights) {
  const PassArgs<LT>& A = EA;
  const int lane = threadIdx.x;
  const int b = blockIdx.x / A.tiles, tile = blockIdx.x % A.tiles;
  const int l = tile * kWave + lane;
  const bool on = l < A.L;
  const int site = on ? l : A.L - 1;
  const double w = site_weight<WT>(weights, b, A.L, site);
  const double won = on ? w : 0.0;
  CostM<QP, DYN> cm;
  cm.load(A.cost, A.Q);
  const size_t tree = (size_t)b * A.ni * A.L * A.Q;
  Rows<QP, DYN> dp, out;
  dp.init(A.dp + tree, A.ni, A.L, A.Q, site);
  out.init(A.outside + tree, A.ni, A.L, A.Q, site);
  const LT* lv = A.leaves + (size_t)b * A.nl * A.L;
  const cptr<int> pl = as_const(A.plan) + (size_t)b * 4 * A.ni;
  const int n_all = A.nl + A.ni;
  double* part = A.part + (size_t)blockIdx.x * n_all * EA.E;
  const int8_t* st = SOFT ? nullptr : EA.states + (size_t)b * A.ni * A.L + site;
  for (int r = 0; r < A.ni; ++r) {
    const I4 e = load_step(pl, r);
    float op[QP], d0[QP], d1[QP], m0[QP], m1[QP];
    out.get(e.x, op);
    inside_row<QP, DYN>(e.y, dp, lv, A.L, site, d0);
    msg<QP, DYN, SOFT>(cm, A.a, A.bcoef, d0, m0);
    inside_row<QP, DYN>(e.z, dp, lv, A.L, site, d1);
    msg<QP, DYN, SOFT>(cm, A.a, A.bcoef, d1, m1);
    int sp = 0;
    if constexpr (!SOFT) sp = st[(size_t)e.x * A.L];
    // the padded path keeps one copy of the edge's code: k is a run-time loop there
    constexpr int kUnrollK = DYN ? 1 : 2;
#pragma unroll kUnrollK
    for (int k = 0; k < 2; ++k) {
      const int desc = k == 0 ? e.y : e.z;
      float base[QP], d[QP];
#pragma unroll
      for (int i = 0; i < QP; ++i) {
        base[i] = op[i] + (k == 0 ? m1[i] : m0[i]);
        d[i] = k == 0 ? d0[i] : d1[i];
      }
      const bool leaf = (desc >> 24) == kKindLeaf;
      int sc = 0;
      if constexpr (!SOFT)
        if (!leaf) sc = st[(size_t)(desc & 0xFFFF) * A.L];
      edge_sums<QP, DYN, SOFT>(cm, A.cost, A.a, base, d, won, sp, leaf, sc,
                               part + (size_t)desc_node(desc, A.nl) * EA.E, lane);
    }
  }
}

// One thread per entry (b, node, q): the tiles' partials summed in tile order.
// The fp64 total goes to tile 0's slot (this thread's own entry: nobody else
// reads it here) for edge_length_kernel, the fp32 value to counts / length_min
// / length_max.  The root's entries are 0 and its partials are not read.
__global__ __launch_bounds__(256) void edge_reduce_kernel(double* __restrict__ part, int B,
                                                          int tiles, int n_all, int E, int QQ,
                                                          float* __restrict__ counts,
                                                          float* __restrict__ length_min,
                                                          float* __restrict__ length_max) {
  const int64_t per = (int64_t)n_all * E;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)B * per) return;
  const int64_t b = t / per, rem = t % per;
  const int64_t node = rem / E;
  const int q = (int)(rem % E);
  double* p = part + b * tiles * per + rem;
  double acc = 0.0;
  if (node != n_all - 1)
    for (int k = 0; k < tiles; ++k) acc += p[(int64_t)k * per];
  p[0] = acc;
  const int64_t edge = b * n_all + node;
  if (q < QQ) counts[edge * QQ + q] = (float)acc;
  else if (q == QQ) length_min[edge] = (float)acc;
  else length_max[edge] = (float)acc;
}

// lengths[b][node] = sum_ij counts[i][j] C[i][j] over the fp64 totals, in entry order
__global__ __launch_bounds__(256) void edge_length_kernel(const double* __restrict__ part,
                                                          const float* __restrict__ cost, int B,
                                                          int tiles, int n_all, int E, int QQ,
                                                          float* __restrict__ lengths) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)B * n_all) return;
  const int64_t b = t / n_all, node = t % n_all;
  const double* p = part + (b * tiles * n_all + node) * E;
  double acc = 0.0;
  for (int q = 0; q < QQ; ++q) acc += p[q] * (double)cost[q];
  lengths[t] = (float)acc;
}

// bytes of the partials at their tau = 0 size; false when a tree's entry
// count does not fit an int or the bytes do not fit int64
bool edge_sizes(int B, int L, int n_all, int Q, int64_t* bytes) {
  const int64_t per_tree = (int64_t)tiles(L) * n_all * ((int64_t)Q * Q + 2);
  if (per_tree > INT_MAX) return false;
  return !__builtin_mul_overflow((int64_t)B, per_tree * 8, bytes);
}

template <class LT>
int edge_run(const PassCall<LT>& c, const int8_t* states, float* counts, float* lengths,
             float* length_min, float* length_max) {
  return run_pass(
      c, c.outside && counts && lengths && c.workspace,
      [&](int64_t& need) {
        const bool rest = states && length_min && length_max;
        if (c.tau > 0.0f ? (states || length_min || length_max) : !rest)
          return set_error(TREX_E_ARG, "%s: states, length_min and length_max must all be given "
                           "at tau = 0 and all be NULL at tau > 0", c.fn);
        need = trex_edge_workspace_bytes(c.B, c.L, c.n_all, c.Q);
        if (need == 0 || (int64_t)c.B * c.n_all * (c.Q * c.Q + 2) > 0x7FFFFFFFLL * 256)
          return set_error(TREX_E_UNSUPPORTED, "%s: B=%d L=%d n_all=%d Q=%d: the workspace is "
                           "too large", c.fn, c.B, c.L, c.n_all, c.Q);
        return TREX_OK;
      },
      0, [&](const PassArgs<LT>& A, hipStream_t st) {
        const bool soft = c.tau > 0.0f;
        const int QQ = c.Q * c.Q, E = QQ + (soft ? 0 : 2);
        const EdgeArgs<LT> EA{A, states, E};
        with_variant(c.Q, soft, c.weights != nullptr, [&](auto v) {
          using V = decltype(v);
          hipLaunchKernelGGL((edge_changes_kernel<LT, V::QP, V::DYN, V::SOFT, V::WT>),
                             dim3(A.B * A.tiles), dim3(kWave), 0, st, EA, c.weights);
        });
        const int64_t n = (int64_t)c.B * c.n_all * E, m = (int64_t)c.B * c.n_all;
        hipLaunchKernelGGL(edge_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                           A.part, c.B, A.tiles, c.n_all, E, QQ, counts, length_min, length_max);
        hipLaunchKernelGGL(edge_length_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st,
                           A.part, c.cost, c.B, A.tiles, c.n_all, E, QQ, lengths);
      });
}

}  // namespace

}  // namespace trex

using namespace trex;

extern "C" int64_t trex_edge_workspace_bytes(int B, int L, int n_all, int Q) {
  int64_t bytes;
  if (!workspace_shape_ok(B, L, n_all, Q) || n_all > 65535) return 0;
  return edge_sizes(B, L, n_all, Q, &bytes) ? bytes : 0;
}

extern "C" int trex_sankoff_edge_changes_w(const int32_t* attach_plan, const int8_t* leaves,
                                           const float* cost, int B, int L, int n_all, int Q,
                                           float tau, const float* dp, const float* outside,
                                           const int8_t* states, const float* weights,
                                           float* counts, float* lengths, float* length_min,
                                           float* length_max, void* workspace,
                                           int64_t workspace_bytes, void* stream) {
  return edge_run<int8_t>({"trex_sankoff_edge_changes_w", attach_plan, leaves, cost, B, L, n_all,
                           Q, tau, dp, const_cast<float*>(outside), weights, nullptr, workspace,
                           workspace_bytes, stream},
                          states, counts, lengths, length_min, length_max);
}

extern "C" int trex_sankoff_sets_edge_changes_w(const int32_t* attach_plan,
                                                const int32_t* leaf_sets, const float* cost,
                                                int B, int L, int n_all, int Q, float tau,
                                                const float* dp, const float* outside,
                                                const int8_t* states, const float* weights,
                                                float* counts, float* lengths, float* length_min,
                                                float* length_max, void* workspace,
                                                int64_t workspace_bytes, void* stream) {
  return edge_run<int32_t>({"trex_sankoff_sets_edge_changes_w", attach_plan, leaf_sets, cost, B,
                            L, n_all, Q, tau, dp, const_cast<float*>(outside), weights, nullptr,
                            workspace, workspace_bytes, stream},
                           states, counts, lengths, length_min, length_max);
}
