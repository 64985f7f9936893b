// State-set leaves (DESIGN.md "State-set leaves"): a leaf's cell is an int32
// bit mask of the states it allows at that site, its inside row 0 where the
// bit is set and 1e5 elsewhere.  Mask 1 << c is code c, mask 0 is code -1
// (all 1e5), (1 << Q) - 1 is missing data (all 0); bits at or above Q are
// never looked at.  Owns trex_sankoff_sets_fwd and its workspace size,
// trex_sankoff_sets_outside, trex_sankoff_sets_nni_w and
// trex_sankoff_sets_attach_w (trex_sankoff_sets_spr_w is in sankoff_spr.hip).
//
// The forward pass is a kernel of its own in the shape of the outside pass
// (sankoff_rows.h): one 64-lane wave takes 64 consecutive sites of ONE tree,
// one lane per site, and walks the attach plan's [n_int][4] records in
// ascending row order -- a post-order, every child id being below its
// parent's.  Per row D_p = M_c0 + M_c1; a child's row comes from its mask
// (leaf) or from the DP-table row this lane wrote earlier (same lane, same
// address).  The outside, NNI and attachment passes are the kernels of
// sankoff_rows.h instantiated for int32 leaves.
#include "sankoff_rows.h"

namespace trex {

namespace {

// The forward's record: the common one (plan: the attach plan) with site_score
// where a pass with an outside table has that, and hard_root behind it.  It
// keeps this layout of its own because moving site_score behind the common
// part changed the padded kernels' SGPR spill counts (PERFLOG.md).
struct SetsFwdArgs {
  const int* plan;
  const int32_t* leaves;
  const float* cost;
  float* dp;
  float* site_score;  // [B][L] or null
  double* part;       // [B][tiles]
  int B, L, nl, ni, Q, tiles;
  float a, bcoef;
  int hard_root;
  SetsFwdArgs(const PassArgs<int32_t>& A, float* site_score_, int hard_root_)
      : plan(A.plan), leaves(A.leaves), cost(A.cost), dp(const_cast<float*>(A.dp)),
        site_score(site_score_), part(A.part), B(A.B), L(A.L), nl(A.nl), ni(A.ni), Q(A.Q),
        tiles(A.tiles), a(A.a), bcoef(A.bcoef), hard_root(hard_root_) {}
};

template <int QP, bool DYN, bool SOFT>
__global__ __launch_bounds__(kWave) void sets_fwd_kernel(const SetsFwdArgs A) {
  const int lane = threadIdx.x;
  const int b = blockIdx.x / A.tiles, tile = blockIdx.x % A.tiles;
  const int l = tile * kWave + lane;
  const bool on = l < A.L;
  const int site = on ? l : A.L - 1;  // tail lanes recompute the last site, store nothing
  CostM<QP, DYN> cm;
  cm.load(A.cost, A.Q);
  Rows<QP, DYN> dp;
  dp.init(A.dp + (size_t)b * A.ni * A.L * A.Q, A.ni, A.L, A.Q, site);
  const int32_t* lv = A.leaves + (size_t)b * A.nl * A.L;
  const cptr<int> pl = as_const(A.plan) + (size_t)b * 4 * A.ni;
  float dn[QP];
  for (int r = 0; r < A.ni; ++r) {
    const I4 e = load_step(pl, r);
    float d[QP], m0[QP], m1[QP];
    inside_row<QP, DYN>(e.y, dp, lv, A.L, site, d);
    message<QP, DYN, SOFT>(cm, A.a, A.bcoef, d, m0);
    inside_row<QP, DYN>(e.z, dp, lv, A.L, site, d);
    message<QP, DYN, SOFT>(cm, A.a, A.bcoef, d, m1);
#pragma unroll
    for (int j = 0; j < QP; ++j) dn[j] = m0[j] + m1[j];
    if (on) dp.put(e.x, dn);
  }
  // dn is the root's row: the plan's last record is the root
  float s;
  if (SOFT && !A.hard_root) s = oplus<QP, DYN, SOFT>(cm, A.a, A.bcoef, dn);
  else s = oplus<QP, DYN, false>(cm, A.a, A.bcoef, dn);
  if (A.site_score && on) A.site_score[(size_t)b * A.L + l] = s;
  const double t = wave_sum_lane0(on ? (double)s : 0.0);
  if (lane == 0) A.part[blockIdx.x] = t;
}

}  // namespace

}  // namespace trex

using namespace trex;

extern "C" int64_t trex_sets_fwd_workspace_bytes(int B, int L, int n_all, int Q) {
  return partials_workspace_bytes(B, L, n_all, Q, 1);  // one entry, the tree's score
}

extern "C" int trex_sankoff_sets_fwd(const int32_t* attach_plan, const int32_t* leaf_sets,
                                     const float* cost, int B, int L, int n_all, int Q, float tau,
                                     unsigned flags, float* dp, float* site_score,
                                     float* tree_score, void* workspace, int64_t workspace_bytes,
                                     void* stream) {
  const PassCall<int32_t> c{"trex_sankoff_sets_fwd", attach_plan, leaf_sets, cost, B, L, n_all, Q,
                            tau, dp, nullptr, nullptr, tree_score, workspace, workspace_bytes,
                            stream};
  return run_pass(
      c, tree_score && workspace,
      [&](int64_t& need) {
        if (flags & ~TREX_FLAG_HARD_ROOT)
          return set_error(TREX_E_ARG, "%s: unknown flags 0x%x", c.fn, flags);
        need = trex_sets_fwd_workspace_bytes(B, L, n_all, Q);
        return TREX_OK;
      },
      1, [&](const PassArgs<int32_t>& A, hipStream_t st) {
        const SetsFwdArgs FA(A, site_score, (flags & TREX_FLAG_HARD_ROOT) ? 1 : 0);
        with_variant(Q, tau > 0.0f, false, [&](auto v) {
          using V = decltype(v);
          hipLaunchKernelGGL((sets_fwd_kernel<V::QP, V::DYN, V::SOFT>), dim3(A.B * A.tiles),
                             dim3(kWave), 0, st, FA);
        });
      });
}

extern "C" int trex_sankoff_sets_outside(const int32_t* nni_plan, const int32_t* leaf_sets,
                                         const float* cost, int B, int L, int n_all, int Q,
                                         float tau, const float* dp, float* outside,
                                         void* stream) {
  return outside_run<int32_t>({"trex_sankoff_sets_outside", nni_plan, leaf_sets, cost, B, L, n_all,
                               Q, tau, dp, outside, nullptr, nullptr, nullptr, 0, stream});
}

extern "C" int trex_sankoff_sets_nni_w(const int32_t* nni_plan, const int32_t* leaf_sets,
                                       const float* cost, int B, int L, int n_all, int Q,
                                       float tau, const float* dp, const float* outside,
                                       const float* weights, float* nni_score, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  return nni_run<int32_t>({"trex_sankoff_sets_nni_w", nni_plan, leaf_sets, cost, B, L, n_all, Q,
                           tau, dp, const_cast<float*>(outside), weights, nni_score, workspace,
                           workspace_bytes, stream});
}

extern "C" int trex_sankoff_sets_attach_w(const int32_t* attach_plan, const int32_t* leaf_sets,
                                          const float* cost, int B, int L, int n_all, int Q,
                                          float tau, const float* dp, const float* outside,
                                          const int32_t* sub_sets, const float* sub_rows,
                                          const float* weights, float* attach_score,
                                          void* workspace, int64_t workspace_bytes,
                                          void* stream) {
  return attach_run<int32_t>({"trex_sankoff_sets_attach_w", attach_plan, leaf_sets, cost, B, L,
                              n_all, Q, tau, dp, const_cast<float*>(outside), weights,
                              attach_score, workspace, workspace_bytes, stream},
                             "sub_sets", sub_sets, sub_rows);
}
