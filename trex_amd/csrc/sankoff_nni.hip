// NNI neighbour scores and attachment scores on the Sankoff DP table for
// leaves given as int8 codes: the entry points over the kernels of
// sankoff_rows.h (DESIGN.md "NNI neighbour scoring", "Attachment scores",
// "Site weights").  sankoff_sets.hip has the same entry points for leaves
// given as state sets.
#include "sankoff_rows.h"

using namespace trex;

extern "C" int trex_sankoff_outside(const int32_t* nni_plan, const int8_t* leaves,
                                    const float* cost, int B, int L, int n_all, int Q, float tau,
                                    const float* dp, float* outside, void* stream) {
  return outside_run("trex_sankoff_outside", nni_plan, leaves, cost, B, L, n_all, Q, tau, dp,
                     outside, stream);
}

extern "C" int64_t trex_nni_workspace_bytes(int B, int L, int n_all, int Q) {
  if (B <= 0 || L <= 0 || n_all < 5 || n_all % 2 == 0 || Q < 2 || Q > kSiteMaxQ) return 0;
  const int64_t ni = n_all - (n_all + 1) / 2;
  return (int64_t)B * ((L + kWave - 1) / kWave) * (ni - 1) * 2 * 8 + 256;
}

extern "C" int trex_sankoff_nni_w(const int32_t* nni_plan, const int8_t* leaves,
                                  const float* cost, int B, int L, int n_all, int Q, float tau,
                                  const float* dp, const float* outside, const float* weights,
                                  float* nni_score, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
  return nni_run("trex_sankoff_nni_w", nni_plan, leaves, cost, B, L, n_all, Q, tau, dp, outside,
                 weights, nni_score, workspace, workspace_bytes, stream);
}

extern "C" int trex_sankoff_nni(const int32_t* nni_plan, const int8_t* leaves, const float* cost,
                                int B, int L, int n_all, int Q, float tau, const float* dp,
                                const float* outside, float* nni_score, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  return nni_run<int8_t>("trex_sankoff_nni", nni_plan, leaves, cost, B, L, n_all, Q, tau, dp,
                         outside, nullptr, nni_score, workspace, workspace_bytes, stream);
}

extern "C" int64_t trex_attach_workspace_bytes(int B, int L, int n_all, int Q) {
  if (B <= 0 || L <= 0 || n_all < 5 || n_all % 2 == 0 || Q < 2 || Q > kSiteMaxQ) return 0;
  return (int64_t)B * ((L + kWave - 1) / kWave) * n_all * 8 + 256;
}

extern "C" int trex_sankoff_attach_w(const int32_t* attach_plan, const int8_t* leaves,
                                     const float* cost, int B, int L, int n_all, int Q, float tau,
                                     const float* dp, const float* outside,
                                     const int8_t* sub_codes, const float* sub_rows,
                                     const float* weights, float* attach_score, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
  return attach_run("trex_sankoff_attach_w", "sub_codes", attach_plan, leaves, cost, B, L, n_all,
                    Q, tau, dp, outside, sub_codes, sub_rows, weights, attach_score, workspace,
                    workspace_bytes, stream);
}

extern "C" int trex_sankoff_attach(const int32_t* attach_plan, const int8_t* leaves,
                                   const float* cost, int B, int L, int n_all, int Q, float tau,
                                   const float* dp, const float* outside, const int8_t* sub_codes,
                                   const float* sub_rows, float* attach_score, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  return attach_run<int8_t>("trex_sankoff_attach", "sub_codes", attach_plan, leaves, cost, B, L,
                            n_all, Q, tau, dp, outside, sub_codes, sub_rows, nullptr, attach_score,
                            workspace, workspace_bytes, stream);
}
