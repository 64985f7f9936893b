// libtrexhip.so -- tree-cost kernels (maraxen/trex src/trex/tree.py) for gfx950.
//
//  a12 update_seq      (tree.py:110-130)  state softmax, fwd + VJP
//  a11 update_tree     (tree.py:50-107)   masked row softmax, fwd + VJP
//  a9  compute_surrogate_cost (tree.py:163-209): G = F F^T (split-K MFMA),
//      loss / dA / M = diag(r+c) - (A+A^T) (one combine pass), dF = M F (MFMA)
//  a10 compute_soft_cost (tree.py:212-266): W = S C per site, G = F W^T
//  a13 enforce_graph_constraints (tree.py:133-160), fwd + grad
//  a8  compute_cost    (tree.py:269-296)  gather-reduce
//  a14 optax adam (+ clip_by_global_norm) fused update
//
// Four translation units, one private header:
//  tree.hip       (this file) the element-wise kernels a8 / a10 - a13, the
//                 combine / constraint / row-sum kernels, the one-workgroup
//                 small surrogate, and the entry points that compose them
//  tree_gram.hip  the Gram G = S S^T: kernels v1 / v2 / v3 / v5, their plans,
//                 gram() with its launch table, the trex_tree_gram* entries
//  tree_mf.hip    dF = M F: kernels v2 / v3 / v5, the leaf codes, mf_x3() with
//                 its launch table, the trex_tree_mf* entries
//  tree_opt.hip   a14 and the fused ancestors' pass: Adam / optax kernels,
//                 the step state, the trex_adam_* / trex_optax_* / trex_step_*
//                 entries
//  tree_dev.h     what two or more of them share
//
// Precision: the optimiser's default GEMMs (gemm="x3") are f16x3 split
// products on v_mfma_f32_32x32x16_f16 (tree_dev.h), held to the f32 path's
// rtol 1e-5 vs fp64; gemm="f32" and the plain entry points (trex_tree_gram,
// trex_tree_mf, trex_tree_surrogate) run exact f32 fmaf chains on
// v_mfma_f32_32x32x2_f32.  All reductions are fixed-order (fp64), so results
// are bitwise reproducible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "tree_dev.h"

namespace trex {
namespace {

// ---------------------------------------------------------------------------
// a12 update_seq: S = softmax_q(T * X) per (ancestor, site)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void update_seq_kernel(const float* __restrict__ x, int64_t rows,
                                                        int Q, float T, float* __restrict__ s) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool al = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(s)) & 15) == 0;
  if (Q == 4 && al) {  // one float4 in, one float4 out per row
    const float4* x4 = reinterpret_cast<const float4*>(x);
    float4* s4 = reinterpret_cast<float4*>(s);
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
      const float4 v = x4[r];
      const float a = v.x * T, b = v.y * T, c = v.z * T, d = v.w * T;
      const float m = fmaxf(fmaxf(a, b), fmaxf(c, d));
      const float ea = expf(a - m), eb = expf(b - m), ec = expf(c - m), ed = expf(d - m);
      const float inv = 1.0f / (((ea + eb) + ec) + ed);
      s4[r] = make_float4(ea * inv, eb * inv, ec * inv, ed * inv);
    }
    return;
  }
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
    const float* xr = x + r * Q;
    float* sr = s + r * Q;
    float m = -INFINITY;
    for (int q = 0; q < Q; ++q) m = fmaxf(m, xr[q] * T);
    float sum = 0.0f;
    for (int q = 0; q < Q; ++q) sum += expf(xr[q] * T - m);
    const float inv = 1.0f / sum;
    for (int q = 0; q < Q; ++q) sr[q] = expf(xr[q] * T - m) * inv;  // one store per element
  }
}

__global__ __launch_bounds__(256) void update_seq_bwd_kernel(const float* __restrict__ s,
                                                            const float* __restrict__ ds,
                                                            int64_t rows, int Q, float T,
                                                            float* __restrict__ dx) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool al = ((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(ds) |
                    reinterpret_cast<uintptr_t>(dx)) & 15) == 0;
  if (Q == 4 && al) {
    const float4* s4 = reinterpret_cast<const float4*>(s);
    const float4* g4 = reinterpret_cast<const float4*>(ds);
    float4* d4 = reinterpret_cast<float4*>(dx);
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
      const float4 a = s4[r], g = g4[r];
      float dot = a.x * g.x;
      dot = fmaf(a.y, g.y, dot);
      dot = fmaf(a.z, g.z, dot);
      dot = fmaf(a.w, g.w, dot);
      d4[r] = make_float4(T * a.x * (g.x - dot), T * a.y * (g.y - dot), T * a.z * (g.z - dot),
                          T * a.w * (g.w - dot));
    }
    return;
  }
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
    const float* sr = s + r * Q;
    const float* gr = ds + r * Q;
    float dot = 0.0f;
    for (int q = 0; q < Q; ++q) dot = fmaf(sr[q], gr[q], dot);
    for (int q = 0; q < Q; ++q) dx[r * Q + q] = T * sr[q] * (gr[q] - dot);
  }
}

// ---------------------------------------------------------------------------
// a11 update_tree: logits z (masked), A = row softmax.  One block per row.
//   theta/noise/gates [N-1][n_anc]; A [N][N]
// ---------------------------------------------------------------------------
__device__ __forceinline__ float tree_logit(const float* theta, const float* noise,
                                            const float* gates, int N, int n_anc, float T, int i,
                                            int j, bool* valid) {
  const int nl = N - n_anc;
  *valid = false;
  if (i == N - 1) {
    if (j == N - 1) { *valid = true; return 1.0f; }
    return -INFINITY;
  }
  if (j < nl) return -INFINITY;
  const int ja = j - nl;
  if (i >= nl && !(ja > i - nl)) return -INFINITY;  // ancestor block: upper triangular
  const size_t k = (size_t)i * n_anc + ja;
  float p = theta[k] + (noise ? noise[k] : 0.0f);
  if (gates) p *= gates[k];
  *valid = true;
  return p / T;
}

__global__ __launch_bounds__(256) void update_tree_kernel(const float* __restrict__ theta,
                                                         const float* __restrict__ noise,
                                                         const float* __restrict__ gates, int N,
                                                         int n_anc, float T, float* __restrict__ A) {
  __shared__ float red[256];
  const int i = blockIdx.x;
  float m = -INFINITY;
  for (int j = threadIdx.x; j < N; j += 256) {
    bool v;
    m = fmaxf(m, tree_logit(theta, noise, gates, N, n_anc, T, i, j, &v));
  }
  red[threadIdx.x] = m;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + w]);
    __syncthreads();
  }
  m = red[0];
  __syncthreads();
  float s = 0.0f;
  for (int j = threadIdx.x; j < N; j += 256) {
    bool v;
    const float z = tree_logit(theta, noise, gates, N, n_anc, T, i, j, &v);
    const float e = v ? expf(z - m) : 0.0f;
    A[(size_t)i * N + j] = e;
    s += e;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  const float inv = 1.0f / red[0];
  for (int j = threadIdx.x; j < N; j += 256) A[(size_t)i * N + j] *= inv;
}

__global__ __launch_bounds__(256) void update_tree_bwd_kernel(const float* __restrict__ A,
                                                             const float* __restrict__ dA,
                                                             const float* __restrict__ gates,
                                                             int N, int n_anc, float T,
                                                             float* __restrict__ dtheta) {
  __shared__ double sh[256];
  const int i = blockIdx.x;  // rows 0..N-2
  const int nl = N - n_anc;
  double dot = 0.0;
  for (int j = threadIdx.x; j < N; j += 256)
    dot += (double)A[(size_t)i * N + j] * (double)dA[(size_t)i * N + j];
  const float d = (float)block_sum_256(dot, sh);
  for (int ja = threadIdx.x; ja < n_anc; ja += 256) {
    const int j = nl + ja;
    const bool valid = (i < nl) || (ja > i - nl);
    float g = 0.0f;
    if (valid) {
      const float a = A[(size_t)i * N + j];
      g = a * (dA[(size_t)i * N + j] - d) / T;
      if (gates) g *= gates[(size_t)i * n_anc + ja];
    }
    dtheta[(size_t)i * n_anc + ja] = g;
  }
}

// ---------------------------------------------------------------------------
// a9 combine: per row i (one block): rowloss_i, dA row, M row.
//   loss = sum_ij A_ij (G_ii + G_jj - 2 G_ij) / 2 ; dA_ij = (G_ii+G_jj)/2 - G_ij
//   M = diag(r + c) - (A + A^T)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void surrogate_combine_kernel(const float* __restrict__ A,
                                                               const float* __restrict__ G, int N,
                                                               float* __restrict__ dA,
                                                               float* __restrict__ M,
                                                               double* __restrict__ rowloss,
                                                               _Float16* __restrict__ M16 = nullptr,
                                                               int ldm = 0, float sm = 1.0f) {
  __shared__ double sh[256];
  const int i = blockIdx.x;
  const float gii = G[(size_t)i * N + i];
  double l = 0.0, rs = 0.0, cs = 0.0;
  for (int j = threadIdx.x; j < N; j += 256) {
    const float a = A[(size_t)i * N + j];
    const float at = A[(size_t)j * N + i];
    const float gjj = G[(size_t)j * N + j];
    const float gij = G[(size_t)i * N + j];
    l += (double)a * ((double)gii + (double)gjj - 2.0 * (double)gij);
    rs += a;
    cs += at;
    if (dA) dA[(size_t)i * N + j] = 0.5f * (gii + gjj) - gij;
  }
  const double L = block_sum_256(l, sh);
  const double rc = block_sum_256(rs, sh) + block_sum_256(cs, sh);
  if (threadIdx.x == 0) rowloss[i] = 0.5 * L;
  if (M) {
    for (int j = threadIdx.x; j < N; j += 256) {
      const float a = A[(size_t)i * N + j] + A[(size_t)j * N + i];
      const float m = (i == j ? (float)rc : 0.0f) - a;
      M[(size_t)i * N + j] = m;
      if (M16) {  // the pre-split copy (split_x3_group layout, zero past N)
        const float v = m * sm;
        const _Float16 hi = (_Float16)v;
        _Float16* g = M16 + ((size_t)i * (ldm / 4) + (j >> 2)) * 8 + (j & 3);
        g[0] = hi;
        g[4] = (_Float16)(v - (float)hi);
      }
    }
    if (M16)
      for (int j = N + threadIdx.x; j < ldm; j += 256) {
        _Float16* g = M16 + ((size_t)i * (ldm / 4) + (j >> 2)) * 8 + (j & 3);
        g[0] = (_Float16)0.0f;
        g[4] = (_Float16)0.0f;
      }
  }
}

// The whole surrogate for small trees (N <= 64, N K <= 4096: the NK eval
// shape is 63 x 30) in one workgroup: S, G = S S^T and M in LDS, G by
// fp32 fmaf over k in order (i <= j computed, mirrored: exactly symmetric),
// the combine's rows in fp64 (thread i sums row i over j in order), the
// loss summed over rows in order by thread 0, dS = M S.  One launch where
// the general path takes five (Gram, its reduce, combine, row sum, MF).
constexpr int kSurSmallN = 64;
constexpr int kSurSmallNK = 4096;
__global__ __launch_bounds__(1024) void surrogate_small_kernel(const float* __restrict__ S,
                                                              const float* __restrict__ A, int N,
                                                              int K, float* __restrict__ loss,
                                                              float* __restrict__ dS,
                                                              float* __restrict__ dA,
                                                              float* __restrict__ G_out) {
  constexpr int T = 1024;
  __shared__ float sS[kSurSmallNK];
  __shared__ float sG[kSurSmallN * kSurSmallN];
  __shared__ float sM[kSurSmallN * kSurSmallN];
  __shared__ float sA[kSurSmallN * kSurSmallN];
  __shared__ double part[3][kSurSmallN * 4];  // row loss, row sum, column sum partials
  __shared__ double rl[kSurSmallN];
  const int tid = threadIdx.x;
  // every operand into LDS first, all loads in flight together; each sum
  // below runs four independent partial chains combined in a fixed order (a
  // serial chain of LDS reads per entry left the block latency-bound)
  for (int e = tid; e < N * K; e += T) sS[e] = S[e];
  for (int e = tid; e < N * N; e += T) sA[e] = A[e];
  __syncthreads();
  auto dot4 = [](const float* x, int sx, const float* y, int sy, int n) {
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
    int t = 0;
    for (; t + 3 < n; t += 4) {
      c0 = fmaf(x[t * sx], y[t * sy], c0);
      c1 = fmaf(x[(t + 1) * sx], y[(t + 1) * sy], c1);
      c2 = fmaf(x[(t + 2) * sx], y[(t + 2) * sy], c2);
      c3 = fmaf(x[(t + 3) * sx], y[(t + 3) * sy], c3);
    }
    for (; t < n; ++t) c0 = fmaf(x[t * sx], y[t * sy], c0);
    return (c0 + c1) + (c2 + c3);
  };
  for (int e = tid; e < N * N; e += T) {
    const int i = e / N, j = e - i * N;
    if (i > j) continue;
    const float g = dot4(sS + i * K, 1, sS + j * K, 1, K);
    sG[i * N + j] = g;
    sG[j * N + i] = g;
  }
  __syncthreads();
  // combine: row i over 4 threads (j = q, q + 4, ...), fp64 partials
  if (tid < 4 * N) {
    const int i = tid >> 2, q = tid & 3;
    const float gii = sG[i * N + i];
    double l = 0.0, rs = 0.0, cs = 0.0;
    for (int j = q; j < N; j += 4) {
      const float a = sA[i * N + j];
      const float at = sA[j * N + i];
      const float gjj = sG[j * N + j];
      const float gij = sG[i * N + j];
      l += (double)a * ((double)gii + (double)gjj - 2.0 * (double)gij);
      rs += a;
      cs += at;
      if (dA) dA[(size_t)i * N + j] = 0.5f * (gii + gjj) - gij;
      sM[i * N + j] = -(a + at);
    }
    part[0][tid] = l;
    part[1][tid] = rs;
    part[2][tid] = cs;
  }
  if (G_out)
    for (int e = tid; e < N * N; e += T) G_out[e] = sG[e];
  __syncthreads();
  if (tid < N) {
    const int i = tid;
    const double* p0 = part[0] + 4 * i;
    const double* p1 = part[1] + 4 * i;
    const double* p2 = part[2] + 4 * i;
    rl[i] = 0.5 * (((p0[0] + p0[1]) + p0[2]) + p0[3]);
    const double rc = (((p1[0] + p1[1]) + p1[2]) + p1[3]) + (((p2[0] + p2[1]) + p2[2]) + p2[3]);
    sM[i * N + i] += (float)rc;
  }
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int i = 0; i < N; ++i) t += rl[i];
    loss[0] = (float)t;
  }
  if (dS)
    for (int e = tid; e < N * K; e += T) {
      const int n = e / K, k = e - n * K;
      dS[e] = dot4(sM + n * N, 1, sS + k, K, N);
    }
}

__global__ __launch_bounds__(256) void sum_rows_kernel(const double* __restrict__ v, int n,
                                                      float scale, float* __restrict__ out,
                                                      int accumulate,
                                                      const StepState* __restrict__ ss = nullptr) {
  __shared__ double sh[256];
  if (ss) scale = ss->T;
  double s = 0.0;
  for (int t = threadIdx.x; t < n; t += 256) s += v[t];
  s = block_sum_256(s, sh);
  if (threadIdx.x == 0) out[0] = (accumulate ? out[0] : 0.0f) + (float)(s * scale);
}

// ---------------------------------------------------------------------------
// a10 W = S C per (node, site):  ckind 0: W = S; 1: W = S * c (vector);
//     2: W = S @ C (matrix, w_j = sum_q s_q C[q][j])
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void weight_seq_kernel(const float* __restrict__ S, int64_t rows,
                                                        int Q, const float* __restrict__ C,
                                                        int ckind, float* __restrict__ W) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows;
       r += (int64_t)gridDim.x * blockDim.x) {
    const float* s = S + r * Q;
    for (int j = 0; j < Q; ++j) {
      float w;
      if (ckind == 0) {
        w = s[j];
      } else if (ckind == 1) {
        w = s[j] * C[j];
      } else {
        w = 0.0f;
        for (int q = 0; q < Q; ++q) w = fmaf(s[q], C[q * Q + j], w);
      }
      W[r * Q + j] = w;
    }
  }
}

// soft-cost combine: loss_i = sum_j A_ij (E_i + E_j - 2 G_ij) / 2, E = diag(G)
// (E_i = sum S_i * W_i = <S_i, W_i>, tree.py:255)
__global__ __launch_bounds__(256) void soft_combine_kernel(const float* __restrict__ A,
                                                          const float* __restrict__ G, int N,
                                                          double* __restrict__ rowloss) {
  __shared__ double sh[256];
  const int i = blockIdx.x;
  const double ei = G[(size_t)i * N + i];
  double l = 0.0;
  for (int j = threadIdx.x; j < N; j += 256)
    l += (double)A[(size_t)i * N + j] *
         (ei + (double)G[(size_t)j * N + j] - 2.0 * (double)G[(size_t)i * N + j]);
  l = block_sum_256(l, sh);
  if (threadIdx.x == 0) rowloss[i] = 0.5 * l;
}

// ---------------------------------------------------------------------------
// a13 constraint: scale * sum_cols (sum_{i<N-1} A[i][c] - 2)^2, c in last n_anc
//   grad (x gscale, accumulated into dA): 2 scale (colsum - 2)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void constraint_kernel(const float* __restrict__ A, int N,
                                                        float scale, float gscale,
                                                        double* __restrict__ colloss,
                                                        float* __restrict__ dA,
                                                        const StepState* __restrict__ ss) {
  __shared__ double sh[256];
  if (ss) gscale = ss->T;
  const int n_anc = (N - 1) / 2;
  const int c = N - n_anc + blockIdx.x;
  double s = 0.0;
  for (int i = threadIdx.x; i < N - 1; i += 256) s += A[(size_t)i * N + c];
  s = block_sum_256(s, sh);
  const double dev = s - 2.0;
  if (threadIdx.x == 0) colloss[blockIdx.x] = (double)scale * dev * dev;
  if (dA) {
    const float g = (float)(2.0 * scale * dev) * gscale;
    for (int i = threadIdx.x; i < N - 1; i += 256) dA[(size_t)i * N + c] += g;
  }
}

// ---------------------------------------------------------------------------
// a8 compute_cost: seq = argmax_q S, parent = argmax_j A (first index), sum
//   subst[seq[parent][l]][seq[i][l]] over i < N-1, l.  One block per node i.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void compute_cost_kernel(const float* __restrict__ S,
                                                          const float* __restrict__ A,
                                                          const float* __restrict__ subst, int N,
                                                          int L, int Q,
                                                          double* __restrict__ rowcost) {
  __shared__ double sh[256];
  __shared__ float bv[256];
  __shared__ int bi[256];
  const int i = blockIdx.x;
  // parent = first argmax of row i
  float best = -INFINITY;
  int arg = 0x7FFFFFFF;
  for (int j = threadIdx.x; j < N; j += 256) {
    const float v = A[(size_t)i * N + j];
    if (v > best || (v == best && j < arg)) { best = v; arg = j; }
  }
  bv[threadIdx.x] = best;
  bi[threadIdx.x] = arg;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      const float v = bv[threadIdx.x + w];
      const int k = bi[threadIdx.x + w];
      if (v > bv[threadIdx.x] || (v == bv[threadIdx.x] && k < bi[threadIdx.x])) {
        bv[threadIdx.x] = v;
        bi[threadIdx.x] = k;
      }
    }
    __syncthreads();
  }
  const int p = bi[0] == 0x7FFFFFFF ? 0 : bi[0];
  double s = 0.0;
  for (int l = threadIdx.x; l < L; l += 256) {
    const float* si = S + ((size_t)i * L + l) * Q;
    const float* sp = S + ((size_t)p * L + l) * Q;
    int a = 0, c = 0;
    float va = si[0], vc = sp[0];
    for (int q = 1; q < Q; ++q) {
      if (si[q] > va) { va = si[q]; a = q; }
      if (sp[q] > vc) { vc = sp[q]; c = q; }
    }
    s += subst[c * Q + a];
  }
  s = block_sum_256(s, sh);
  if (threadIdx.x == 0) rowcost[i] = s;
}

// loss = rows (x 1) then + cols x gscale: the two sum_rows_kernel launches of
// trex_tree_surrogate_combine + trex_tree_constraint in one, same arithmetic
__global__ __launch_bounds__(256) void sum_rows2_kernel(const double* __restrict__ v1, int n1,
                                                       const double* __restrict__ v2, int n2,
                                                       float scale2, float* __restrict__ out,
                                                       const StepState* __restrict__ ss) {
  __shared__ double sh[256];
  if (ss) scale2 = ss->T;
  double s = 0.0;
  for (int t = threadIdx.x; t < n1; t += 256) s += v1[t];
  s = block_sum_256(s, sh);
  double s2 = 0.0;
  for (int t = threadIdx.x; t < n2; t += 256) s2 += v2[t];
  s2 = block_sum_256(s2, sh);
  if (threadIdx.x == 0) {
    const float first = 0.0f + (float)(s * 1.0f);
    out[0] = first + (float)(s2 * scale2);
  }
}

__global__ __launch_bounds__(256) void identity_kernel(int N, float* __restrict__ A) {
  const size_t total = (size_t)N * N;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256)
    A[t] = (t / N == t % N) ? 1.0f : 0.0f;
}

// discretize_tree_topology: one_hot(argmax(A[i]), n_nodes), first index on ties
__global__ __launch_bounds__(256) void discretize_kernel(const float* __restrict__ A, int ncols,
                                                        int n_nodes, float* __restrict__ out) {
  __shared__ float bv[256];
  __shared__ int bi[256];
  const int i = blockIdx.x;
  float best = -INFINITY;
  int arg = 0x7FFFFFFF;
  for (int j = threadIdx.x; j < ncols; j += 256) {
    const float v = A[(size_t)i * ncols + j];
    if (v > best || (v == best && j < arg)) { best = v; arg = j; }
  }
  bv[threadIdx.x] = best;
  bi[threadIdx.x] = arg;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      const float v = bv[threadIdx.x + w];
      const int k = bi[threadIdx.x + w];
      if (v > bv[threadIdx.x] || (v == bv[threadIdx.x] && k < bi[threadIdx.x])) {
        bv[threadIdx.x] = v;
        bi[threadIdx.x] = k;
      }
    }
    __syncthreads();
  }
  const int a = bi[0] == 0x7FFFFFFF ? 0 : bi[0];
  for (int j = threadIdx.x; j < n_nodes; j += 256) out[(size_t)i * n_nodes + j] = (j == a) ? 1.0f : 0.0f;
}

}  // namespace

int grid_for(int64_t n, int per, int cap) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, cap));
}

// power of two s with max_abs * s <= 2^14 (f16 split headroom)
float split_scale(float max_abs) {
  if (!pos_finite_f32(max_abs)) return 1.0f;
  return std::ldexp(1.0f, 14 - (int)std::ceil(std::log2((double)max_abs)));
}

}  // namespace trex

using namespace trex;

extern "C" int trex_tree_update_seq(const float* x, int n_anc, int L, int Q, float T, float* s,
                                    void* stream) {
  if (!x || !s || n_anc < 0 || L <= 0 || Q <= 0)
    return set_error(TREX_E_ARG, "trex_tree_update_seq: bad arguments");
  const int64_t rows = (int64_t)n_anc * L;
  if (rows == 0) return TREX_OK;
  hipLaunchKernelGGL(update_seq_kernel, dim3(grid_for(rows)), dim3(256), 0, (hipStream_t)stream,
                     x, rows, Q, T, s);
  return hip_check("trex_tree_update_seq");
}

extern "C" int trex_tree_update_seq_bwd(const float* s, const float* ds, int n_anc, int L, int Q,
                                        float T, float* dx, void* stream) {
  if (!s || !ds || !dx || n_anc < 0 || L <= 0 || Q <= 0)
    return set_error(TREX_E_ARG, "trex_tree_update_seq_bwd: bad arguments");
  const int64_t rows = (int64_t)n_anc * L;
  if (rows == 0) return TREX_OK;
  hipLaunchKernelGGL(update_seq_bwd_kernel, dim3(grid_for(rows)), dim3(256), 0,
                     (hipStream_t)stream, s, ds, rows, Q, T, dx);
  return hip_check("trex_tree_update_seq_bwd");
}

extern "C" int trex_tree_update_tree(const float* theta, const float* noise, const float* gates,
                                     int N, int n_anc, float T, float* A, void* stream) {
  if (!A || N < 2 || n_anc < 0 || n_anc >= N || !pos_finite_f32(T))
    return set_error(TREX_E_ARG, "trex_tree_update_tree: bad arguments");
  if (n_anc > 0 && !theta) return set_error(TREX_E_ARG, "trex_tree_update_tree: theta is NULL");
  if (n_anc == 0) {  // tree.py:68-69: identity
    hipLaunchKernelGGL(identity_kernel, dim3(grid_for((int64_t)N * N)), dim3(256), 0,
                       (hipStream_t)stream, N, A);
    return hip_check("trex_tree_update_tree");
  }
  hipLaunchKernelGGL(update_tree_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, theta, noise,
                     gates, N, n_anc, T, A);
  return hip_check("trex_tree_update_tree");
}

extern "C" int trex_tree_update_tree_bwd(const float* A, const float* dA, const float* gates,
                                         int N, int n_anc, float T, float* dtheta, void* stream) {
  if (!A || !dA || !dtheta || N < 2 || n_anc <= 0 || n_anc >= N || !pos_finite_f32(T))
    return set_error(TREX_E_ARG, "trex_tree_update_tree_bwd: bad arguments");
  hipLaunchKernelGGL(update_tree_bwd_kernel, dim3(N - 1), dim3(256), 0, (hipStream_t)stream, A,
                     dA, gates, N, n_anc, T, dtheta);
  return hip_check("trex_tree_update_tree_bwd");
}

extern "C" int trex_tree_surrogate(const float* S, const float* A, int N, int64_t K, float* loss,
                                   float* dS, float* dA, float* G_out, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  if (!S || !A || !loss || !workspace || N <= 0 || K <= 0 || K > 0x7FFFFFFF)
    return set_error(TREX_E_ARG, "trex_tree_surrogate: bad arguments");
  if (workspace_bytes < trex_tree_workspace_bytes(N, K))
    return set_error(TREX_E_ARG, "trex_tree_surrogate: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  char* w = static_cast<char*>(workspace);
  float* part = reinterpret_cast<float*>(w);
  w += part_bytes(N, K);
  float* G = reinterpret_cast<float*>(w);
  w += (int64_t)N * N * 4;
  float* M = reinterpret_cast<float*>(w);
  w += (int64_t)N * N * 4;
  double* rowloss = reinterpret_cast<double*>(w);
  if (N <= kSurSmallN && (int64_t)N * K <= kSurSmallNK) {
    hipLaunchKernelGGL(surrogate_small_kernel, dim3(1), dim3(1024), 0, st, S, A, N, (int)K, loss,
                       dS, dA, G_out);
    return hip_check("trex_tree_surrogate");
  }
  if (int e = gram(S, S, N, K, 1, G, part, st)) return e;
  hipLaunchKernelGGL(surrogate_combine_kernel, dim3(N), dim3(256), 0, st, A, G, N, dA,
                     dS ? M : nullptr, rowloss);
  hipLaunchKernelGGL(sum_rows_kernel, dim3(1), dim3(256), 0, st, rowloss, N, 1.0f, loss, 0,
                     (const StepState*)nullptr);
  if (dS) launch_mf2(M, S, N, (int)K, 0, N, dS, st);
  if (G_out &&
      hipMemcpyAsync(G_out, G, sizeof(float) * (size_t)N * N, hipMemcpyDeviceToDevice, st) !=
          hipSuccess)
    return hip_check("trex_tree_surrogate(G)");
  return hip_check("trex_tree_surrogate");
}

extern "C" int trex_tree_soft_cost(const float* S, const float* A, const float* C, int ckind,
                                   int N, int L, int Q, float* loss, float* W_scratch,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
  const int64_t K = (int64_t)L * Q;
  if (!S || !A || !loss || !workspace || N <= 0 || L <= 0 || Q <= 0 || ckind < 0 || ckind > 2 ||
      (ckind > 0 && !C) || (ckind > 0 && !W_scratch))
    return set_error(TREX_E_ARG, "trex_tree_soft_cost: bad arguments");
  if (workspace_bytes < trex_tree_workspace_bytes(N, K))
    return set_error(TREX_E_ARG, "trex_tree_soft_cost: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  char* w = static_cast<char*>(workspace);
  float* part = reinterpret_cast<float*>(w);
  w += part_bytes(N, K);
  float* G = reinterpret_cast<float*>(w);
  w += (int64_t)N * N * 8;
  double* rowloss = reinterpret_cast<double*>(w);
  const float* Wp = S;
  if (ckind > 0) {
    const int64_t rows = (int64_t)N * L;
    hipLaunchKernelGGL(weight_seq_kernel, dim3(grid_for(rows)), dim3(256), 0, st, S, rows, Q, C,
                       ckind, W_scratch);
    Wp = W_scratch;
  }
  // G[i][j] = <S_i, W_j> (not symmetric for a general C): all tile pairs
  if (int e = gram(S, Wp, N, K, ckind == 0 ? 1 : 0, G, part, st)) return e;
  hipLaunchKernelGGL(soft_combine_kernel, dim3(N), dim3(256), 0, st, A, G, N, rowloss);
  hipLaunchKernelGGL(sum_rows_kernel, dim3(1), dim3(256), 0, st, rowloss, N, 1.0f, loss, 0,
                     (const StepState*)nullptr);
  return hip_check("trex_tree_soft_cost");
}

extern "C" int trex_tree_constraint(const float* A, int N, float scale, float grad_scale,
                                    float* loss, int accumulate, float* dA, void* workspace,
                                    void* stream) {
  if (!A || !loss || !workspace || N < 3)
    return set_error(TREX_E_ARG, "trex_tree_constraint: bad arguments");
  const int n_anc = (N - 1) / 2;
  hipStream_t st = (hipStream_t)stream;
  double* colloss = static_cast<double*>(workspace);
  hipLaunchKernelGGL(constraint_kernel, dim3(n_anc), dim3(256), 0, st, A, N, scale, grad_scale,
                     colloss, dA, (const StepState*)nullptr);
  hipLaunchKernelGGL(sum_rows_kernel, dim3(1), dim3(256), 0, st, colloss, n_anc, grad_scale,
                     loss, accumulate, (const StepState*)nullptr);
  return hip_check("trex_tree_constraint");
}

extern "C" int trex_tree_constraint_dev(const float* A, int N, float scale, const void* state,
                                        float* loss, int accumulate, float* dA, void* workspace,
                                        void* stream) {
  if (!A || !loss || !workspace || !state || N < 3)
    return set_error(TREX_E_ARG, "trex_tree_constraint_dev: bad arguments");
  const int n_anc = (N - 1) / 2;
  hipStream_t st = (hipStream_t)stream;
  double* colloss = static_cast<double*>(workspace);
  const StepState* ss = static_cast<const StepState*>(state);
  hipLaunchKernelGGL(constraint_kernel, dim3(n_anc), dim3(256), 0, st, A, N, scale, 0.0f, colloss,
                     dA, ss);
  hipLaunchKernelGGL(sum_rows_kernel, dim3(1), dim3(256), 0, st, colloss, n_anc, 0.0f, loss,
                     accumulate, ss);
  return hip_check("trex_tree_constraint_dev");
}

extern "C" int trex_tree_compute_cost(const float* S, const float* A, const float* subst, int N,
                                      int L, int Q, float* cost, void* workspace, void* stream) {
  if (!S || !A || !subst || !cost || !workspace || N < 2 || L <= 0 || Q <= 0)
    return set_error(TREX_E_ARG, "trex_tree_compute_cost: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  double* rowcost = static_cast<double*>(workspace);
  // rows 0..N-2 only ([:-1] in tree.py:296)
  hipLaunchKernelGGL(compute_cost_kernel, dim3(N - 1), dim3(256), 0, st, S, A, subst, N, L, Q,
                     rowcost);
  hipLaunchKernelGGL(sum_rows_kernel, dim3(1), dim3(256), 0, st, rowcost, N - 1, 1.0f, cost, 0,
                     (const StepState*)nullptr);
  return hip_check("trex_tree_compute_cost");
}

extern "C" int trex_tree_discretize(const float* A, int nrows, int ncols, int n_nodes, float* out,
                                    void* stream) {
  if (!A || !out || nrows <= 0 || ncols <= 0 || n_nodes <= 0)
    return set_error(TREX_E_ARG, "trex_tree_discretize: bad arguments");
  hipLaunchKernelGGL(discretize_kernel, dim3(nrows), dim3(256), 0, (hipStream_t)stream, A, ncols,
                     n_nodes, out);
  return hip_check("trex_tree_discretize");
}

extern "C" int trex_tree_surrogate_constraint(const float* A, const float* G, int N, float scale,
                                              float grad_scale, const void* state, float* loss,
                                              float* dA, float* M, float max_abs_m, void* M16,
                                              int ldm16, void* workspace, void* stream) {
  if (!A || !G || !loss || !dA || !M || !workspace || N < 3 ||
      (M16 && (ldm16 < N || ldm16 % 4 != 0 || !pos_finite_f32(max_abs_m))))
    return set_error(TREX_E_ARG, "trex_tree_surrogate_constraint: bad arguments");
  const int n_anc = (N - 1) / 2;
  hipStream_t st = (hipStream_t)stream;
  double* rowloss = static_cast<double*>(workspace);
  double* colloss = rowloss + N;
  const StepState* ss = static_cast<const StepState*>(state);
  hipLaunchKernelGGL(surrogate_combine_kernel, dim3(N), dim3(256), 0, st, A, G, N, dA, M,
                     rowloss, static_cast<_Float16*>(M16), ldm16,
                     M16 ? split_scale(max_abs_m) : 1.0f);
  hipLaunchKernelGGL(constraint_kernel, dim3(n_anc), dim3(256), 0, st, A, N, scale, grad_scale,
                     colloss, dA, ss);
  hipLaunchKernelGGL(sum_rows2_kernel, dim3(1), dim3(256), 0, st, rowloss, N, colloss, n_anc,
                     grad_scale, loss, ss);
  return hip_check("trex_tree_surrogate_constraint");
}

extern "C" int trex_tree_surrogate_combine(const float* A, const float* G, int N, float* loss,
                                           float* dA, float* M, void* workspace, void* stream) {
  if (!A || !G || !loss || !workspace || N <= 0)
    return set_error(TREX_E_ARG, "trex_tree_surrogate_combine: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  double* rowloss = static_cast<double*>(workspace);
  hipLaunchKernelGGL(surrogate_combine_kernel, dim3(N), dim3(256), 0, st, A, G, N, dA, M,
                     rowloss);
  hipLaunchKernelGGL(sum_rows_kernel, dim3(1), dim3(256), 0, st, rowloss, N, 1.0f, loss, 0,
                     (const StepState*)nullptr);
  return hip_check("trex_tree_surrogate_combine");
}
