// SPR neighbour scores on the Sankoff DP and outside tables (DESIGN.md "SPR
// neighbour scoring"; definitions: include/trex_hip.h), for leaves given as
// int8 codes and as int32 state sets, over the row helpers of sankoff_rows.h.
//
// Move (v, x) prunes the subtree of v (u = v's parent disappears, v's sibling
// s takes its place) and regrafts it on the edge above x.  One 64-lane wave
// takes 64 consecutive sites of ONE tree and loops over the n_all - 1 pruned
// nodes; per pruned node
//   (a) the path sweep walks from g = parent(u) up to the root and writes the
//       changed inside rows D'_y of u's proper ancestors P,
//   (b) the walk visits the internal nodes p of T\v in pre-order: both child
//       edges of p from O'_p and the children's messages (two scores), and
//       the children's outside rows O'_c.
// Every internal node has at most one changed row -- D' on P, O' off it --
// kept in a scratch area [B * tiles][n_int][64 lanes][Q] of the workspace.
// The layout is lane-private: a lane only reads a scratch row the same lane
// stored earlier in program order (same address), so no barrier, fence or
// cache-policy bit is needed; tail lanes own their slots, recompute the last
// site and are kept out of the sums by a select.  The plan (plan.cpp, SPR
// plan) gives per node its parent, sibling and pre-order entry / exit; whether
// a node is in subtree(v) or on the path, and so which table a row comes
// from, is decided with scalar compares (wave-uniform).  Site scores are
// summed over the wave in fp64 (fixed butterfly), lane 0 writes the per-tile
// partials, reduce_partials_kernel adds the tiles in order.  The entries of
// moves that do not exist get +inf partials on every call.  Owns
// trex_spr_workspace_bytes, trex_sankoff_spr_w and trex_sankoff_sets_spr_w.
#include <climits>

#include "sankoff_rows.h"

namespace trex {

namespace {

template <class LT>
struct SprArgs : PassArgs<LT> {
  float* scratch;  // [B * tiles][ni][64][Q]
};

// inside row of node id x in T: a leaf's from its cell, else the DP table's
template <int QP, bool DYN, class LT>
__device__ __forceinline__ void node_row(int x, int nl, const Rows<QP, DYN>& dp,
                                         const LT* __restrict__ tree_leaves, int L, int site,
                                         float (&d)[QP]) {
  if (x < nl) leaf_row<QP>(tree_leaves[(size_t)x * L + site], d);
  else dp.get(x - nl, d);
}

// message() of sankoff_rows.h.  The kernel below has eleven message sites in
// three nested loops; on the padded path each site unrolls to 20 x 20 guarded
// terms, so there the message is one out-of-line function per (SOFT, TRANS)
// that every site calls -- the same arithmetic, a fraction of the code.  The
// Q <= 4 instantiations inline it as the sibling kernels do.
template <int QP, bool SOFT, bool TRANS>
__device__ __noinline__ void message_padded(const CostM<QP, true>& cm, float a, float bcoef,
                                            const float (&d)[QP], float (&m)[QP]) {
  message<QP, true, SOFT, TRANS>(cm, a, bcoef, d, m);
}
template <int QP, bool DYN, bool SOFT, bool TRANS = false>
__device__ __forceinline__ void msg(const CostM<QP, DYN>& cm, float a, float bcoef,
                                    const float (&d)[QP], float (&m)[QP]) {
  if constexpr (DYN) message_padded<QP, SOFT, TRANS>(cm, a, bcoef, d, m);
  else message<QP, DYN, SOFT, TRANS>(cm, a, bcoef, d, m);
}

template <class LT, int QP, bool DYN, bool SOFT, bool WT>
__global__ __launch_bounds__(kWave) void spr_score_kernel(const SprArgs<LT> SA,
                                                          const float* weights) {
  const PassArgs<LT>& A = SA;
  const int lane = threadIdx.x;
  const int b = blockIdx.x / A.tiles, tile = blockIdx.x % A.tiles;
  const int l = tile * kWave + lane;
  const bool on = l < A.L;
  const int site = on ? l : A.L - 1;
  const double w = site_weight<WT>(weights, b, A.L, site);
  CostM<QP, DYN> cm;
  cm.load(A.cost, A.Q);
  const size_t tree = (size_t)b * A.ni * A.L * A.Q;
  Rows<QP, DYN> dp, out, scr;
  dp.init(A.dp + tree, A.ni, A.L, A.Q, site);
  out.init(A.outside + tree, A.ni, A.L, A.Q, site);
  scr.init(SA.scratch + (size_t)blockIdx.x * A.ni * kWave * A.Q, A.ni, kWave, A.Q, lane);
  const LT* lv = A.leaves + (size_t)b * A.nl * A.L;
  const int nl = A.nl, n_all = A.nl + A.ni;
  const int* tree_plan = A.plan + (size_t)b * (12 * A.ni + 4);
  const cptr<int> node = as_const(tree_plan);
  const cptr<int> walk = node + 4 * n_all;
  double* part = A.part + (size_t)blockIdx.x * (n_all - 1) * n_all;
  for (int v = 0; v < n_all - 1; ++v) {
    const I4 nv = load_step(node, v);  // u, s, v's entry and exit
    const int u = nv.x, s = nv.y;
    const I4 nu = load_step(node, u);  // g, t, u's entry
    const int g = nu.x, tu = nu.z;
    double* pv = part + (size_t)v * n_all;
    // moves that do not exist: x in subtree(v), x = u
    for (int x = lane; x < n_all; x += kWave) {
      const int tx = tree_plan[4 * x + 2];
      if (x == u || (tx >= nv.z && tx < nv.w)) pv[x] = INFINITY;
    }
    float mv[QP], dr[QP];  // M_v; the inside row of T\v's root
    {
      float d[QP];
      node_row<QP, DYN>(v, nl, dp, lv, A.L, site, d);
      msg<QP, DYN, SOFT>(cm, A.a, A.bcoef, d, mv);
    }
    // (a) D' on the proper ancestors of u, bottom-up; the last one is the root's
    if (g < 0) {
      node_row<QP, DYN>(s, nl, dp, lv, A.L, site, dr);
    } else {
      float d[QP], ma[QP], mb[QP];
      node_row<QP, DYN>(s, nl, dp, lv, A.L, site, d);
      msg<QP, DYN, SOFT>(cm, A.a, A.bcoef, d, ma);
      int y = g, sib = nu.y;
      for (;;) {
        node_row<QP, DYN>(sib, nl, dp, lv, A.L, site, d);
        msg<QP, DYN, SOFT>(cm, A.a, A.bcoef, d, mb);
#pragma unroll
        for (int j = 0; j < QP; ++j) dr[j] = ma[j] + mb[j];
        scr.put(y - nl, dr);
        const I4 ny = load_step(node, y);
        if (ny.x < 0) break;
        msg<QP, DYN, SOFT>(cm, A.a, A.bcoef, dr, ma);
        y = ny.x;
        sib = ny.y;
      }
    }
    {  // x = the root of T\v: w is the new root
      float md[QP], x[QP];
      msg<QP, DYN, SOFT>(cm, A.a, A.bcoef, dr, md);
#pragma unroll
      for (int i = 0; i < QP; ++i) x[i] = md[i] + mv[i];
      const float sr = oplus<QP, DYN, SOFT>(cm, A.a, A.bcoef, x);
      const double s2 = wave_sum_lane0(on ? (double)sr * w : 0.0);
      if (lane == 0) pv[g < 0 ? s : n_all - 1] = s2;
    }
    // (b) the internal nodes of T\v in pre-order
    for (int k = 0; k < A.ni; ++k) {
      const I4 e = load_step(walk, k);
      const int p = nl + e.x;
      const I4 np = load_step(node, p);
      if (p == u || (np.z >= nv.z && np.z < nv.w)) continue;  // u is gone; subtree(v) is pruned
      const bool p_path = np.z <= tu && tu < np.w;             // p in P (p != u)
      float op[QP];
      if (g < 0 && p == s) {  // the root of T\v
#pragma unroll
        for (int j = 0; j < QP; ++j) op[j] = 0.0f;
      } else if (p_path) {
        out.get(e.x, op);
      } else {
        scr.get(e.x, op);
      }
      // p's children in T\v: s stands where u stood
      const int c0 = e.y == u ? s : e.y, c1 = e.z == u ? s : e.z;
      const I4 n0 = load_step(node, c0), n1 = load_step(node, c1);
      const bool path0 = n0.z <= tu && tu < n0.w, path1 = n1.z <= tu && tu < n1.w;
      float d[QP], m0[QP], m1[QP];
      if (path0) scr.get(c0 - nl, d);
      else node_row<QP, DYN>(c0, nl, dp, lv, A.L, site, d);
      msg<QP, DYN, SOFT>(cm, A.a, A.bcoef, d, m0);
      if (path1) scr.get(c1 - nl, d);
      else node_row<QP, DYN>(c1, nl, dp, lv, A.L, site, d);
      msg<QP, DYN, SOFT>(cm, A.a, A.bcoef, d, m1);
      float sc[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        // the edge above child j: w takes child j and v, p keeps the other child
        float dw[QP], mdw[QP], x[QP];
#pragma unroll
        for (int i = 0; i < QP; ++i) dw[i] = (j == 0 ? m0[i] : m1[i]) + mv[i];
        msg<QP, DYN, SOFT>(cm, A.a, A.bcoef, dw, mdw);
#pragma unroll
        for (int i = 0; i < QP; ++i) x[i] = op[i] + (j == 0 ? m1[i] : m0[i]) + mdw[i];
        sc[j] = oplus<QP, DYN, SOFT>(cm, A.a, A.bcoef, x);
      }
      const double s0 = wave_sum_lane0(on ? (double)sc[0] * w : 0.0);
      const double s1 = wave_sum_lane0(on ? (double)sc[1] * w : 0.0);
      if (lane == 0) {
        pv[c0] = s0;
        pv[c1] = s1;
      }
      // O' of the internal children off the path (on it: O' = O, the table's)
      if (c0 >= nl && !path0) {
        float t[QP], oc[QP];
#pragma unroll
        for (int i = 0; i < QP; ++i) t[i] = op[i] + m1[i];
        msg<QP, DYN, SOFT, true>(cm, A.a, A.bcoef, t, oc);
        scr.put(c0 - nl, oc);
      }
      if (c1 >= nl && !path1) {
        float t[QP], oc[QP];
#pragma unroll
        for (int i = 0; i < QP; ++i) t[i] = op[i] + m0[i];
        msg<QP, DYN, SOFT, true>(cm, A.a, A.bcoef, t, oc);
        scr.put(c1 - nl, oc);
      }
    }
  }
}

// bytes of the per-tile partials, rounded up to 256 (the scratch rows start
// there); false when a size does not fit int64 / the entry count an int
bool spr_sizes(int B, int L, int n_all, int Q, int64_t* part_bytes, int64_t* total) {
  const int64_t nw = (int64_t)B * tiles(L), moves = spr_moves(n_all);
  int64_t part, scr;
  if (moves > INT_MAX || (int64_t)B * moves > 0x7FFFFFFFLL * 256) return false;
  if (__builtin_mul_overflow(nw, moves * 8, &part) ||
      __builtin_add_overflow(part, (int64_t)255, &part))
    return false;
  part = part / 256 * 256;
  if (__builtin_mul_overflow(nw, (int64_t)tree_ni(n_all) * kWave * Q * 4, &scr) ||
      __builtin_add_overflow(part, scr, total) ||
      __builtin_add_overflow(*total, (int64_t)256, total))
    return false;
  *part_bytes = part;
  return true;
}

template <class LT>
int spr_run(const PassCall<LT>& c) {
  int64_t part_bytes = 0;
  return run_pass(
      c, c.outside && c.score && c.workspace,
      [&](int64_t& need) {
        if (!spr_sizes(c.B, c.L, c.n_all, c.Q, &part_bytes, &need))
          return set_error(TREX_E_UNSUPPORTED, "%s: B=%d L=%d n_all=%d: the score table or the "
                           "workspace is too large", c.fn, c.B, c.L, c.n_all);
        return TREX_OK;
      },
      (int)spr_moves(c.n_all), [&](const PassArgs<LT>& A, hipStream_t st) {
        const SprArgs<LT> SA{
            A, reinterpret_cast<float*>(static_cast<char*>(c.workspace) + part_bytes)};
        with_variant(c.Q, c.tau > 0.0f, c.weights != nullptr, [&](auto v) {
          using V = decltype(v);
          hipLaunchKernelGGL((spr_score_kernel<LT, V::QP, V::DYN, V::SOFT, V::WT>),
                             dim3(A.B * A.tiles), dim3(kWave), 0, st, SA, c.weights);
        });
      });
}

}  // namespace

}  // namespace trex

using namespace trex;

extern "C" int64_t trex_spr_workspace_bytes(int B, int L, int n_all, int Q) {
  int64_t part_bytes, total;
  if (!workspace_shape_ok(B, L, n_all, Q) || n_all > 65535) return 0;
  return spr_sizes(B, L, n_all, Q, &part_bytes, &total) ? total : 0;
}

extern "C" int trex_sankoff_spr_w(const int32_t* spr_plan, const int8_t* leaves,
                                  const float* cost, int B, int L, int n_all, int Q, float tau,
                                  const float* dp, const float* outside, const float* weights,
                                  float* spr_score, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
  return spr_run<int8_t>({"trex_sankoff_spr_w", spr_plan, leaves, cost, B, L, n_all, Q, tau, dp,
                          const_cast<float*>(outside), weights, spr_score, workspace,
                          workspace_bytes, stream});
}

extern "C" int trex_sankoff_sets_spr_w(const int32_t* spr_plan, const int32_t* leaf_sets,
                                       const float* cost, int B, int L, int n_all, int Q,
                                       float tau, const float* dp, const float* outside,
                                       const float* weights, float* spr_score, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  return spr_run<int32_t>({"trex_sankoff_sets_spr_w", spr_plan, leaf_sets, cost, B, L, n_all, Q,
                           tau, dp, const_cast<float*>(outside), weights, spr_score, workspace,
                           workspace_bytes, stream});
}
