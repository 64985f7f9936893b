// libtrexhip.so -- the tree-cost optimiser kernels (tree.hip has the map of
// the tree-cost files): optax Adam / AdamW / SGD / RMSprop with optional
// global-norm clip (a14), update_tree's VJP fused with the tree parameters'
// Adam step, the ancestors' pass (update_seq VJP + Adam + the next
// update_seq in one kernel) and the device step state of a captured loop.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "tree_dev.h"

namespace trex {
namespace {

// ---------------------------------------------------------------------------
// a14 optax adam (b1, b2, eps; eps_root = 0) with optional global-norm clip
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sq_norm_kernel(const float* __restrict__ g, int64_t n,
                                                     double* __restrict__ part) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256)
    s += (double)g[t] * (double)g[t];
  s = block_sum_256(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p,
                                                  const float* __restrict__ g,
                                                  float* __restrict__ mu, float* __restrict__ nu,
                                                  int64_t n, float lr, float b1, float b2,
                                                  float eps, float bc1, float bc2,
                                                  const double* __restrict__ sqnorm,
                                                  int nparts, float clip,
                                                  const StepState* __restrict__ ss) {
  if (ss) {
    bc1 = ss->bc1;
    bc2 = ss->bc2;
  }
  float scale = 1.0f;
  if (sqnorm) {
    double s = 0.0;
    for (int k = 0; k < nparts; ++k) s += sqnorm[k];  // same fixed order in every thread
    const float norm = (float)sqrt(s);
    if (!(norm < clip)) scale = clip / norm;
  }
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
    const float gt = (scale == 1.0f) ? g[t] : (g[t] / (clip / scale)) * clip;
    const float m = (1.0f - b1) * gt + b1 * mu[t];
    const float v = (1.0f - b2) * (gt * gt) + b2 * nu[t];
    mu[t] = m;
    nu[t] = v;
    const float mh = m / bc1;
    const float vh = v / bc2;
    p[t] = p[t] + (-lr) * (mh / (sqrtf(vh) + eps));
  }
}

// update_tree's VJP (update_tree_bwd_kernel's arithmetic) with the
// tree_params' Adam step (adam_kernel's, no clip) applied in the same pass:
// one block per row, the gradient optionally written out as well
__global__ __launch_bounds__(256) void update_tree_bwd_adam_kernel(
    const float* __restrict__ A, const float* __restrict__ dA, const float* __restrict__ gates,
    int N, int n_anc, float T, float* __restrict__ dtheta, float* __restrict__ p,
    float* __restrict__ mu, float* __restrict__ nu, float lr, float b1, float b2, float eps,
    float bc1, float bc2, const StepState* __restrict__ ss) {
  __shared__ double sh[256];
  if (ss) {
    bc1 = ss->bc1;
    bc2 = ss->bc2;
  }
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
    const size_t t = (size_t)i * n_anc + ja;
    if (dtheta) dtheta[t] = g;
    const float m = (1.0f - b1) * g + b1 * mu[t];
    const float v = (1.0f - b2) * (g * g) + b2 * nu[t];
    mu[t] = m;
    nu[t] = v;
    const float mh = m / bc1;
    const float vh = v / bc2;
    p[t] = p[t] + (-lr) * (mh / (sqrtf(vh) + eps));
  }
}

// optax transformations of src/trex/evals/benchmark.py:41-72
// (create_optimizer), optionally after clip_by_global_norm:
//   kind 0 adam(lr, b1, b2, eps)        s1 = mu, s2 = nu (bias-corrected)
//   kind 1 adamw(lr, ..., wd)           adam + wd * p, then * -lr
//   kind 2 sgd(lr, momentum = b1)       s1 = trace: t = g + b1 t
//   kind 3 rmsprop(lr, decay = b2, eps) s2 = nu = b2 nu + (1 - b2) g^2,
//                                       update g / sqrt(nu + eps)
// (optax 0.2.6 defaults: eps_root 0, nesterov off, rmsprop eps inside sqrt,
// initial_scale 0, not centred).
__global__ __launch_bounds__(256) void optax_kernel(int kind, float* __restrict__ p,
                                                   const float* __restrict__ g,
                                                   float* __restrict__ s1,
                                                   float* __restrict__ s2, int64_t n, float lr,
                                                   float b1, float b2, float eps, float wd,
                                                   float bc1, float bc2,
                                                   const double* __restrict__ sqnorm,
                                                   int nparts, float clip,
                                                   const StepState* __restrict__ ss) {
  if (ss) {
    bc1 = ss->bc1;
    bc2 = ss->bc2;
  }
  float scale = 1.0f;
  if (sqnorm) {
    double sum = 0.0;
    for (int k = 0; k < nparts; ++k) sum += sqnorm[k];  // same fixed order in every thread
    const float norm = (float)sqrt(sum);
    if (!(norm < clip)) scale = clip / norm;
  }
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
    const float gt = (scale == 1.0f) ? g[t] : (g[t] / (clip / scale)) * clip;
    float u;
    if (kind <= 1) {
      const float m = (1.0f - b1) * gt + b1 * s1[t];
      const float v = (1.0f - b2) * (gt * gt) + b2 * s2[t];
      s1[t] = m;
      s2[t] = v;
      u = (m / bc1) / (sqrtf(v / bc2) + eps);
      if (kind == 1) u = u + wd * p[t];
    } else if (kind == 2) {
      u = gt + b1 * s1[t];
      s1[t] = u;
    } else {
      const float v = (1.0f - b2) * (gt * gt) + b2 * s2[t];
      s2[t] = v;
      u = gt / sqrtf(v + eps);
    }
    p[t] = p[t] + (-lr) * u;
  }
}

// update_seq VJP fused into the optax Adam update of the ancestor logits
// (no clip): g = T s (ds - <s, ds>) per (ancestor, site) row of Q states,
// then the same Adam arithmetic as adam_kernel; g never touches HBM unless
// g_out is given.  Q = 4 rows move as float4.
template <int QT>
__global__ __launch_bounds__(256) void adam_seq_kernel(const float* __restrict__ s,
                                                      const float* __restrict__ ds, int64_t rows,
                                                      int Qr, float T, float* __restrict__ p,
                                                      float* __restrict__ mu,
                                                      float* __restrict__ nu, float lr, float b1,
                                                      float b2, float eps, float bc1, float bc2,
                                                      float* __restrict__ g_out) {
  const int Q = QT ? QT : Qr;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256) {
    float sv[QT ? QT : 32], gv[QT ? QT : 32];
    if constexpr (QT == 4) {
      const float4 a = reinterpret_cast<const float4*>(s)[r];
      const float4 d = reinterpret_cast<const float4*>(ds)[r];
      sv[0] = a.x; sv[1] = a.y; sv[2] = a.z; sv[3] = a.w;
      gv[0] = d.x; gv[1] = d.y; gv[2] = d.z; gv[3] = d.w;
    } else {
      for (int q = 0; q < Q; ++q) {
        sv[q] = s[r * Q + q];
        gv[q] = ds[r * Q + q];
      }
    }
    float dot = sv[0] * gv[0];
    for (int q = 1; q < Q; ++q) dot = fmaf(sv[q], gv[q], dot);
    float pv[QT ? QT : 32], mv[QT ? QT : 32], vv[QT ? QT : 32];
    if constexpr (QT == 4) {
      const float4 a = reinterpret_cast<const float4*>(p)[r];
      const float4 m = reinterpret_cast<const float4*>(mu)[r];
      const float4 v = reinterpret_cast<const float4*>(nu)[r];
      pv[0] = a.x; pv[1] = a.y; pv[2] = a.z; pv[3] = a.w;
      mv[0] = m.x; mv[1] = m.y; mv[2] = m.z; mv[3] = m.w;
      vv[0] = v.x; vv[1] = v.y; vv[2] = v.z; vv[3] = v.w;
    } else {
      for (int q = 0; q < Q; ++q) {
        pv[q] = p[r * Q + q];
        mv[q] = mu[r * Q + q];
        vv[q] = nu[r * Q + q];
      }
    }
    for (int q = 0; q < Q; ++q) {
      const float gt = T * sv[q] * (gv[q] - dot);
      gv[q] = gt;
      const float m = (1.0f - b1) * gt + b1 * mv[q];
      const float v = (1.0f - b2) * (gt * gt) + b2 * vv[q];
      mv[q] = m;
      vv[q] = v;
      pv[q] = pv[q] + (-lr) * ((m / bc1) / (sqrtf(v / bc2) + eps));
    }
    if constexpr (QT == 4) {
      reinterpret_cast<float4*>(p)[r] = make_float4(pv[0], pv[1], pv[2], pv[3]);
      reinterpret_cast<float4*>(mu)[r] = make_float4(mv[0], mv[1], mv[2], mv[3]);
      reinterpret_cast<float4*>(nu)[r] = make_float4(vv[0], vv[1], vv[2], vv[3]);
      if (g_out) reinterpret_cast<float4*>(g_out)[r] = make_float4(gv[0], gv[1], gv[2], gv[3]);
    } else {
      for (int q = 0; q < Q; ++q) {
        p[r * Q + q] = pv[q];
        mu[r * Q + q] = mv[q];
        nu[r * Q + q] = vv[q];
        if (g_out) g_out[r * Q + q] = gv[q];
      }
    }
  }
}

// One ancestor-logits step with update_seq folded in on both sides: s =
// softmax(T p) recomputed from the logits it reads anyway (the same
// arithmetic as update_seq_kernel, so bitwise the S the step's GEMMs used),
// the VJP g = T s (ds - <s, ds>), the Adam update of p / mu / nu, and the
// NEXT step's S rows softmax(Tn p_new) written to s_out: per row of Q
// logits 16 B of ds + 12 B of Adam state in, 16 B + 12 B out, no separate
// update_seq pass (which re-read p) and no read of the old S.
__device__ __forceinline__ void softmaxq(const float* x, int Q, float T, float* o) {
  float m = -INFINITY;
  for (int q = 0; q < Q; ++q) m = fmaxf(m, x[q] * T);
  float sum = 0.0f;
  for (int q = 0; q < Q; ++q) sum += expf(x[q] * T - m);
  const float inv = 1.0f / sum;
  for (int q = 0; q < Q; ++q) o[q] = expf(x[q] * T - m) * inv;
}

// any Q <= 32 (a grid-stride loop over rows)
__global__ __launch_bounds__(256) void adam_seq_update_kernel(
    const float* __restrict__ ds, int64_t rows, int Q, float T, float Tn, float* __restrict__ p,
    float* __restrict__ mu, float* __restrict__ nu, float lr, float b1, float b2, float eps,
    float bc1, float bc2, float* __restrict__ s_out, const StepState* __restrict__ ss) {
  if (ss) {
    bc1 = ss->bc1;
    bc2 = ss->bc2;
    T = ss->T;
    Tn = ss->Tn;
  }
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256) {
    float pv[32], mv[32], vv[32], gv[32], sv[32];
    for (int q = 0; q < Q; ++q) {
      pv[q] = p[r * Q + q];
      gv[q] = ds[r * Q + q];
      mv[q] = mu[r * Q + q];
      vv[q] = nu[r * Q + q];
    }
    softmaxq(pv, Q, T, sv);
    float dot = sv[0] * gv[0];
    for (int q = 1; q < Q; ++q) dot = fmaf(sv[q], gv[q], dot);
    for (int q = 0; q < Q; ++q) {
      const float gt = T * sv[q] * (gv[q] - dot);
      const float m = (1.0f - b1) * gt + b1 * mv[q];
      const float v = (1.0f - b2) * (gt * gt) + b2 * vv[q];
      mv[q] = m;
      vv[q] = v;
      pv[q] = pv[q] + (-lr) * ((m / bc1) / (sqrtf(v / bc2) + eps));
    }
    softmaxq(pv, Q, Tn, sv);
    for (int q = 0; q < Q; ++q) {
      p[r * Q + q] = pv[q];
      mu[r * Q + q] = mv[q];
      nu[r * Q + q] = vv[q];
      s_out[r * Q + q] = sv[q];
    }
  }
}

__device__ __forceinline__ void softmax4(const float (&x)[4], float T, float (&o)[4]) {
  const float a = x[0] * T, b = x[1] * T, c = x[2] * T, d = x[3] * T;
  const float m = fmaxf(fmaxf(a, b), fmaxf(c, d));
  const float ea = expf(a - m), eb = expf(b - m), ec = expf(c - m), ed = expf(d - m);
  const float inv = 1.0f / (((ea + eb) + ec) + ed);
  o[0] = ea * inv; o[1] = eb * inv; o[2] = ec * inv; o[3] = ed * inv;
}

// One ancestor row (Q = 4) of the fused update_seq VJP + Adam + next
// update_seq: s = softmax(T p) (bitwise the S the step's GEMMs used), g = T s
// (ds - <s, ds>), Adam on p / m / v, s = softmax(Tn p_new).
__device__ __forceinline__ void adam_seq_row4(const float (&gv)[4], float (&pv)[4], float (&mv)[4],
                                              float (&vv)[4], float T, float Tn, float lr,
                                              float b1, float b2, float eps, float bc1, float bc2,
                                              float (&sv)[4]) {
  softmax4(pv, T, sv);
  float dot = sv[0] * gv[0];
#pragma unroll
  for (int q = 1; q < 4; ++q) dot = fmaf(sv[q], gv[q], dot);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float gt = T * sv[q] * (gv[q] - dot);
    const float m = (1.0f - b1) * gt + b1 * mv[q];
    const float v = (1.0f - b2) * (gt * gt) + b2 * vv[q];
    mv[q] = m;
    vv[q] = v;
    pv[q] = pv[q] + (-lr) * ((m / bc1) / (sqrtf(v / bc2) + eps));
  }
  softmax4(pv, Tn, sv);
}

// b^n by squaring in IEEE double: the host entry points and
// trex_step_advance compute the same bits (no pow() implementations to
// disagree, no contraction under -ffp-contract=off)
__host__ __device__ inline double ipow_d(double b, int n) {
  double r = 1.0;
  while (n > 0) {
    if (n & 1) r = r * b;
    b = b * b;
    n >>= 1;
  }
  return r;
}
__host__ __device__ inline float bias_corr(float b, int count) {
  return (float)(1.0 - ipow_d((double)b, count));
}

__global__ void step_advance_kernel(StepState* __restrict__ st, float b1, float b2,
                                    const float* __restrict__ temps, int64_t n_temps) {
  const int k = st->count + 1;
  st->count = k;
  st->bc1 = bias_corr(b1, k);
  st->bc2 = bias_corr(b2, k);
  if (temps && n_temps > 0) {
    st->T = temps[(int64_t)k - 1 < n_temps ? k - 1 : n_temps - 1];
    st->Tn = temps[(int64_t)k < n_temps ? k : n_temps - 1];
  }
}

// Q = 4 (16-B rows): one row per thread over a full grid, every stream
// nontemporal -- 1.63 GB per C5 step touched once, so it should not
// displace anything in L2 / MALL (C5: 329 -> 272 us, 4.9 -> 6.0 TB/s; two or
// four rows per thread, or temporal accesses, were slower: DESIGN §9)
constexpr int kAdamBlock = 256;  // threads per block of the Q = 4 ancestors' pass
// the pass of row r = its thread's index: p / mu / nu updated in place, the
// next S row left in s4 for the caller's store; false past the last row
__device__ __forceinline__ bool adam_seq_update4_row(
    const fv4* __restrict__ ds, int64_t rows, float T, float Tn, fv4* __restrict__ p,
    fv4* __restrict__ mu, fv4* __restrict__ nu, float lr, float b1, float b2, float eps,
    float bc1, float bc2, const StepState* __restrict__ ss, int64_t& r, float (&s4)[4]) {
  if (ss) {
    bc1 = ss->bc1;
    bc2 = ss->bc2;
    T = ss->T;
    Tn = ss->Tn;
  }
  r = (int64_t)blockIdx.x * kAdamBlock + threadIdx.x;
  if (r >= rows) return false;
  const fv4 d = __builtin_nontemporal_load(ds + r), a = __builtin_nontemporal_load(p + r);
  const fv4 m = __builtin_nontemporal_load(mu + r), v = __builtin_nontemporal_load(nu + r);
  float p4[4], g4[4], m4[4], v4[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    p4[q] = a[q];
    g4[q] = d[q];
    m4[q] = m[q];
    v4[q] = v[q];
  }
  adam_seq_row4(g4, p4, m4, v4, T, Tn, lr, b1, b2, eps, bc1, bc2, s4);
  __builtin_nontemporal_store((fv4){p4[0], p4[1], p4[2], p4[3]}, p + r);
  __builtin_nontemporal_store((fv4){m4[0], m4[1], m4[2], m4[3]}, mu + r);
  __builtin_nontemporal_store((fv4){v4[0], v4[1], v4[2], v4[3]}, nu + r);
  return true;
}

// (two kernel names, not one template: profiles and PERFLOG quote them)
__global__ __launch_bounds__(kAdamBlock) void adam_seq_update4_kernel(
    const fv4* __restrict__ ds, int64_t rows, float T, float Tn, fv4* __restrict__ p,
    fv4* __restrict__ mu, fv4* __restrict__ nu, float lr, float b1, float b2, float eps,
    float bc1, float bc2, fv4* __restrict__ s_out, const StepState* __restrict__ ss) {
  int64_t r;
  float s4[4];
  if (!adam_seq_update4_row(ds, rows, T, Tn, p, mu, nu, lr, b1, b2, eps, bc1, bc2, ss, r, s4))
    return;
  __builtin_nontemporal_store((fv4){s4[0], s4[1], s4[2], s4[3]}, s_out + r);
}

// the same pass writing the next S rows pre-split (x3p)
__global__ __launch_bounds__(kAdamBlock) void adam_seq_update4_x3p_kernel(
    const fv4* __restrict__ ds, int64_t rows, float T, float Tn, fv4* __restrict__ p,
    fv4* __restrict__ mu, fv4* __restrict__ nu, float lr, float b1, float b2, float eps,
    float bc1, float bc2, float sx, fv4* __restrict__ s_out, const StepState* __restrict__ ss) {
  int64_t r;
  float s4[4];
  if (!adam_seq_update4_row(ds, rows, T, Tn, p, mu, nu, lr, b1, b2, eps, bc1, bc2, ss, r, s4))
    return;
  // the next S rows (pre-split) stay cacheable: the next step's Gram and MF
  // read them (C5 x3 step 0.640-0.652 -> 0.624-0.628 ms same box against a
  // nontemporal store, PERFLOG)
  s_out[r] = __builtin_bit_cast(fv4, split_x3_group(s4[0], s4[1], s4[2], s4[3], sx));
}

void launch_adam_seq(const float* ds, int64_t rows, int Q, float T, float Tn, float* p, float* mu,
                     float* nu, float lr, float b1, float b2, float eps, float bc1, float bc2,
                     float* s_out, const StepState* ss, hipStream_t st) {
  const bool al = ((reinterpret_cast<uintptr_t>(ds) | reinterpret_cast<uintptr_t>(p) |
                    reinterpret_cast<uintptr_t>(mu) | reinterpret_cast<uintptr_t>(nu) |
                    reinterpret_cast<uintptr_t>(s_out)) & 15) == 0;
  if (Q == 4 && al && rows <= 0x7FFFFFFFLL * 256)
    hipLaunchKernelGGL(adam_seq_update4_kernel, dim3((unsigned)((rows + kAdamBlock - 1) / kAdamBlock)), dim3(kAdamBlock), 0,
                       st, reinterpret_cast<const fv4*>(ds), rows, T, Tn,
                       reinterpret_cast<fv4*>(p), reinterpret_cast<fv4*>(mu),
                       reinterpret_cast<fv4*>(nu), lr, b1, b2, eps, bc1, bc2,
                       reinterpret_cast<fv4*>(s_out), ss);
  else
    hipLaunchKernelGGL(adam_seq_update_kernel, dim3(grid_for(rows)), dim3(256), 0, st, ds, rows, Q,
                       T, Tn, p, mu, nu, lr, b1, b2, eps, bc1, bc2, s_out, ss);
}
}  // namespace
}  // namespace trex

using namespace trex;

extern "C" int trex_adam_step(float* params, const float* grads, float* mu, float* nu, int64_t n,
                              int count, float lr, float b1, float b2, float eps,
                              const double* grad_sq_norm_parts, int n_parts, float clip_norm,
                              void* stream) {
  if (!params || !grads || !mu || !nu || n < 0 || count < 1)
    return set_error(TREX_E_ARG, "trex_adam_step: bad arguments");
  const float bc1 = bias_corr(b1, count);
  const float bc2 = bias_corr(b2, count);
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, params,
                     grads, mu, nu, n, lr, b1, b2, eps, bc1, bc2, grad_sq_norm_parts, n_parts,
                     clip_norm, (const StepState*)nullptr);
  return hip_check("trex_adam_step");
}

extern "C" int trex_step_state_bytes(void) { return (int)sizeof(StepState); }

extern "C" int trex_step_advance(void* state, float b1, float b2, const float* temps,
                                 int64_t n_temps, void* stream) {
  if (!state || (temps && n_temps <= 0))
    return set_error(TREX_E_ARG, "trex_step_advance: bad arguments");
  hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream,
                     static_cast<StepState*>(state), b1, b2, temps, n_temps);
  return hip_check("trex_step_advance");
}

extern "C" int trex_tree_update_tree_bwd_adam(const float* A, const float* dA, const float* gates,
                                              int N, int n_anc, float T, float* dtheta,
                                              float* params, float* mu, float* nu, int count,
                                              const void* state, float lr, float b1, float b2,
                                              float eps, void* stream) {
  if (!A || !dA || !params || !mu || !nu || N < 2 || n_anc <= 0 || n_anc >= N ||
      !pos_finite_f32(T) || (!state && count < 1))
    return set_error(TREX_E_ARG, "trex_tree_update_tree_bwd_adam: bad arguments");
  const float bc1 = state ? 1.0f : bias_corr(b1, count);
  const float bc2 = state ? 1.0f : bias_corr(b2, count);
  hipLaunchKernelGGL(update_tree_bwd_adam_kernel, dim3(N - 1), dim3(256), 0, (hipStream_t)stream,
                     A, dA, gates, N, n_anc, T, dtheta, params, mu, nu, lr, b1, b2, eps, bc1, bc2,
                     static_cast<const StepState*>(state));
  return hip_check("trex_tree_update_tree_bwd_adam");
}

extern "C" int trex_adam_step_dev(float* params, const float* grads, float* mu, float* nu,
                                  int64_t n, const void* state, float lr, float b1, float b2,
                                  float eps, const double* grad_sq_norm_parts, int n_parts,
                                  float clip_norm, void* stream) {
  if (!params || !grads || !mu || !nu || n < 0 || !state)
    return set_error(TREX_E_ARG, "trex_adam_step_dev: bad arguments");
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, params,
                     grads, mu, nu, n, lr, b1, b2, eps, 1.0f, 1.0f, grad_sq_norm_parts, n_parts,
                     clip_norm, static_cast<const StepState*>(state));
  return hip_check("trex_adam_step_dev");
}

extern "C" int trex_optax_step(int kind, float* params, const float* grads, float* state1,
                               float* state2, int64_t n, int count, float lr, float b1, float b2,
                               float eps, float weight_decay, const double* grad_sq_norm_parts,
                               int n_parts, float clip_norm, void* stream) {
  if (kind < 0 || kind > 3 || !params || !grads || n < 0 || count < 1 ||
      ((kind != 3) && !state1) || ((kind != 2) && !state2))
    return set_error(TREX_E_ARG, "trex_optax_step: bad arguments");
  const float bc1 = bias_corr(b1, count);
  const float bc2 = bias_corr(b2, count);
  hipLaunchKernelGGL(optax_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, kind,
                     params, grads, state1, state2, n, lr, b1, b2, eps, weight_decay, bc1, bc2,
                     grad_sq_norm_parts, n_parts, clip_norm, (const StepState*)nullptr);
  return hip_check("trex_optax_step");
}

extern "C" int trex_optax_step_dev(int kind, float* params, const float* grads, float* state1,
                                   float* state2, int64_t n, const void* state, float lr, float b1,
                                   float b2, float eps, float weight_decay,
                                   const double* grad_sq_norm_parts, int n_parts, float clip_norm,
                                   void* stream) {
  if (kind < 0 || kind > 3 || !params || !grads || n < 0 || !state ||
      ((kind != 3) && !state1) || ((kind != 2) && !state2))
    return set_error(TREX_E_ARG, "trex_optax_step_dev: bad arguments");
  hipLaunchKernelGGL(optax_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, kind,
                     params, grads, state1, state2, n, lr, b1, b2, eps, weight_decay, 1.0f, 1.0f,
                     grad_sq_norm_parts, n_parts, clip_norm, static_cast<const StepState*>(state));
  return hip_check("trex_optax_step_dev");
}

extern "C" int trex_adam_seq_step(const float* s_anc, const float* ds_anc, int n_anc, int L,
                                  int Q, float temperature, float* params, float* mu, float* nu,
                                  int count, float lr, float b1, float b2, float eps,
                                  float* grads_out, void* stream) {
  if (!s_anc || !ds_anc || !params || !mu || !nu || n_anc <= 0 || L <= 0 || Q < 2 || Q > 32 ||
      count < 1 || !pos_finite_f32(temperature))
    return set_error(TREX_E_ARG, "trex_adam_seq_step: bad arguments");
  const float bc1 = bias_corr(b1, count);
  const float bc2 = bias_corr(b2, count);
  const int64_t rows = (int64_t)n_anc * L;
  const bool al = ((reinterpret_cast<uintptr_t>(s_anc) | reinterpret_cast<uintptr_t>(ds_anc) |
                    reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(mu) |
                    reinterpret_cast<uintptr_t>(nu) | reinterpret_cast<uintptr_t>(grads_out)) &
                   15) == 0;
  hipStream_t st = (hipStream_t)stream;
  if (Q == 4 && al)
    hipLaunchKernelGGL(adam_seq_kernel<4>, dim3(grid_for(rows)), dim3(256), 0, st, s_anc, ds_anc,
                       rows, Q, temperature, params, mu, nu, lr, b1, b2, eps, bc1, bc2, grads_out);
  else
    hipLaunchKernelGGL(adam_seq_kernel<0>, dim3(grid_for(rows)), dim3(256), 0, st, s_anc, ds_anc,
                       rows, Q, temperature, params, mu, nu, lr, b1, b2, eps, bc1, bc2, grads_out);
  return hip_check("trex_adam_seq_step");
}

extern "C" int trex_adam_seq_update_step(const float* ds_anc, int n_anc, int L, int Q,
                                         float temperature, float next_temperature,
                                         float* params, float* mu, float* nu, int count, float lr,
                                         float b1, float b2, float eps, float* s_next,
                                         void* stream) {
  if (!ds_anc || !params || !mu || !nu || !s_next || n_anc <= 0 || L <= 0 || Q < 2 || Q > 32 ||
      count < 1 || !pos_finite_f32(temperature) || !pos_finite_f32(next_temperature))
    return set_error(TREX_E_ARG, "trex_adam_seq_update_step: bad arguments");
  const float bc1 = bias_corr(b1, count);
  const float bc2 = bias_corr(b2, count);
  const int64_t rows = (int64_t)n_anc * L;
  launch_adam_seq(ds_anc, rows, Q, temperature, next_temperature, params, mu, nu, lr, b1, b2, eps,
                  bc1, bc2, s_next, nullptr, (hipStream_t)stream);
  return hip_check("trex_adam_seq_update_step");
}

extern "C" int trex_adam_seq_update_step_dev(const float* ds_anc, int n_anc, int L, int Q,
                                             const void* state, float* params, float* mu,
                                             float* nu, float lr, float b1, float b2, float eps,
                                             float* s_next, void* stream) {
  if (!ds_anc || !params || !mu || !nu || !s_next || !state || n_anc <= 0 || L <= 0 || Q < 2 ||
      Q > 32)
    return set_error(TREX_E_ARG, "trex_adam_seq_update_step_dev: bad arguments");
  const int64_t rows = (int64_t)n_anc * L;
  launch_adam_seq(ds_anc, rows, Q, 1.0f, 1.0f, params, mu, nu, lr, b1, b2, eps, 1.0f, 1.0f, s_next,
                  static_cast<const StepState*>(state), (hipStream_t)stream);
  return hip_check("trex_adam_seq_update_step_dev");
}

extern "C" int trex_adam_seq_update_step_x3p(const float* ds_anc, int n_anc, int L, int Q,
                                             float temperature, float next_temperature,
                                             float* params, float* mu, float* nu, int count,
                                             float lr, float b1, float b2, float eps,
                                             const void* state, float max_abs_s, void* s16_next,
                                             void* stream) {
  if (!ds_anc || !params || !mu || !nu || !s16_next || n_anc <= 0 || L <= 0 || Q != 4 ||
      !pos_finite_f32(max_abs_s) ||
      (!state && (count < 1 || !pos_finite_f32(temperature) ||
                  !pos_finite_f32(next_temperature))) ||
      ((reinterpret_cast<uintptr_t>(ds_anc) | reinterpret_cast<uintptr_t>(params) |
        reinterpret_cast<uintptr_t>(mu) | reinterpret_cast<uintptr_t>(nu) |
        reinterpret_cast<uintptr_t>(s16_next)) & 15) != 0)
    return set_error(TREX_E_ARG, "trex_adam_seq_update_step_x3p: bad arguments");
  const int64_t rows = (int64_t)n_anc * L;
  const float bc1 = state ? 1.0f : bias_corr(b1, count);
  const float bc2 = state ? 1.0f : bias_corr(b2, count);
  hipLaunchKernelGGL(adam_seq_update4_x3p_kernel, dim3((unsigned)((rows + kAdamBlock - 1) / kAdamBlock)), dim3(kAdamBlock),
                     0, (hipStream_t)stream, reinterpret_cast<const fv4*>(ds_anc), rows,
                     temperature, next_temperature, reinterpret_cast<fv4*>(params),
                     reinterpret_cast<fv4*>(mu), reinterpret_cast<fv4*>(nu), lr, b1, b2, eps, bc1,
                     bc2, split_scale(max_abs_s), static_cast<fv4*>(s16_next),
                     static_cast<const StepState*>(state));
  return hip_check("trex_adam_seq_update_step_x3p");
}

extern "C" int trex_sq_norm_parts(const float* x, int64_t n, double* parts, int n_parts,
                                  void* stream) {
  if (!x || !parts || n_parts <= 0 || n_parts > 8192)
    return set_error(TREX_E_ARG, "trex_sq_norm_parts: bad arguments");
  hipLaunchKernelGGL(sq_norm_kernel, dim3(n_parts), dim3(256), 0, (hipStream_t)stream, x, n,
                     parts);
  return hip_check("trex_sq_norm_parts");
}
