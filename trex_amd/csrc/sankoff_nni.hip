// The row passes of sankoff_rows.h for leaves given as int8 codes (DESIGN.md
// "NNI neighbour scoring", "Attachment scores", "Site weights").  Owns
// trex_sankoff_outside, trex_sankoff_nni / _nni_w, trex_sankoff_attach /
// _attach_w and the two workspace sizes that both leaf types share,
// trex_nni_workspace_bytes and trex_attach_workspace_bytes.  The state-set
// twins are in sankoff_sets.hip, both SPR entry points in sankoff_spr.hip.
#include "sankoff_rows.h"

using namespace trex;

extern "C" int trex_sankoff_outside(const int32_t* nni_plan, const int8_t* leaves,
                                    const float* cost, int B, int L, int n_all, int Q, float tau,
                                    const float* dp, float* outside, void* stream) {
  return outside_run<int8_t>({"trex_sankoff_outside", nni_plan, leaves, cost, B, L, n_all, Q, tau,
                              dp, outside, nullptr, nullptr, nullptr, 0, stream});
}

extern "C" int64_t trex_nni_workspace_bytes(int B, int L, int n_all, int Q) {
  return partials_workspace_bytes(B, L, n_all, Q, nni_moves(n_all));
}

extern "C" int trex_sankoff_nni_w(const int32_t* nni_plan, const int8_t* leaves,
                                  const float* cost, int B, int L, int n_all, int Q, float tau,
                                  const float* dp, const float* outside, const float* weights,
                                  float* nni_score, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
  return nni_run<int8_t>({"trex_sankoff_nni_w", nni_plan, leaves, cost, B, L, n_all, Q, tau, dp,
                          const_cast<float*>(outside), weights, nni_score, workspace,
                          workspace_bytes, stream});
}

extern "C" int trex_sankoff_nni(const int32_t* nni_plan, const int8_t* leaves, const float* cost,
                                int B, int L, int n_all, int Q, float tau, const float* dp,
                                const float* outside, float* nni_score, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  return nni_run<int8_t>({"trex_sankoff_nni", nni_plan, leaves, cost, B, L, n_all, Q, tau, dp,
                          const_cast<float*>(outside), nullptr, nni_score, workspace,
                          workspace_bytes, stream});
}

extern "C" int64_t trex_attach_workspace_bytes(int B, int L, int n_all, int Q) {
  return partials_workspace_bytes(B, L, n_all, Q, attach_moves(n_all));
}

extern "C" int trex_sankoff_attach_w(const int32_t* attach_plan, const int8_t* leaves,
                                     const float* cost, int B, int L, int n_all, int Q, float tau,
                                     const float* dp, const float* outside,
                                     const int8_t* sub_codes, const float* sub_rows,
                                     const float* weights, float* attach_score, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
  return attach_run<int8_t>({"trex_sankoff_attach_w", attach_plan, leaves, cost, B, L, n_all, Q,
                             tau, dp, const_cast<float*>(outside), weights, attach_score,
                             workspace, workspace_bytes, stream},
                            "sub_codes", sub_codes, sub_rows);
}

extern "C" int trex_sankoff_attach(const int32_t* attach_plan, const int8_t* leaves,
                                   const float* cost, int B, int L, int n_all, int Q, float tau,
                                   const float* dp, const float* outside, const int8_t* sub_codes,
                                   const float* sub_rows, float* attach_score, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  return attach_run<int8_t>({"trex_sankoff_attach", attach_plan, leaves, cost, B, L, n_all, Q,
                             tau, dp, const_cast<float*>(outside), nullptr, attach_score,
                             workspace, workspace_bytes, stream},
                            "sub_codes", sub_codes, sub_rows);
}
