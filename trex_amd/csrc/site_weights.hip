// Weighted total of a forward pass's site scores (DESIGN.md "Site weights"):
//   tree_score[b] = sum_l weights[b][l] * site_score[b][l]
// One 256-thread block per tree.  Thread t takes sites t, t + 256, ... in
// ascending order: product and partial sum in fp64; the 256 partials are then
// folded through LDS in a fixed order (stride 128, 64, ... 1) and rounded to
// fp32 once.  No atomics: repeated calls are bitwise equal.
#include <hip/hip_runtime.h>

#include "trex_common.h"

namespace trex {

namespace {

constexpr int kWsumThreads = 256;

__global__ __launch_bounds__(kWsumThreads) void site_weighted_sum_kernel(
    const float* __restrict__ site_score, const float* __restrict__ weights, int L,
    float* __restrict__ tree_score) {
  __shared__ double part[kWsumThreads];
  const int t = threadIdx.x;
  const size_t row = (size_t)blockIdx.x * L;
  double acc = 0.0;
  for (int l = t; l < L; l += kWsumThreads)
    acc += (double)weights[row + l] * (double)site_score[row + l];
  part[t] = acc;
  __syncthreads();
#pragma unroll
  for (int s = kWsumThreads / 2; s > 0; s >>= 1) {
    if (t < s) part[t] += part[t + s];
    __syncthreads();
  }
  if (t == 0) tree_score[blockIdx.x] = (float)part[0];
}

}  // namespace

}  // namespace trex

using namespace trex;

extern "C" int trex_site_weighted_sum(const float* site_score, const float* weights, int B, int L,
                                      float* tree_score, void* stream) {
  const char* fn = "trex_site_weighted_sum";
  if (B <= 0 || L <= 0) return set_error(TREX_E_ARG, "%s: bad shape B=%d L=%d", fn, B, L);
  if (!site_score || !weights || !tree_score)
    return set_error(TREX_E_ARG, "%s: null pointer argument", fn);
  hipLaunchKernelGGL(site_weighted_sum_kernel, dim3((unsigned)B), dim3(kWsumThreads), 0,
                     (hipStream_t)stream, site_score, weights, L, tree_score);
  return hip_check(fn);
}
