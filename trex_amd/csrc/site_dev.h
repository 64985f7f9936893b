// What the two lane-per-site translation units share (sankoff_site.hip: one
// wave per 64 sites; sankoff_site2.hip: a wave pair): the kernel arguments
// and their host fill (over fill_common), the LDS sizes, the bf16 split, the
// barrier, the stamp macro and two prologue pieces.  The row I/O, mat-vec,
// adjoint and dC code differs between the mappings and stays in each kernel.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "sankoff_dev.h"
#include "trex_common.h"
#include "wide_dev.h"

namespace trex {
namespace {

constexpr int kSQ = kSiteSQ;                  // states of a site (Q padded to 20)
constexpr int kSlotF = kSQ * kWave;           // floats per slot / scratch vector
constexpr int kTabF = (kSQ + 1) * kSQ + kSQ;  // leaf messages T[Q + 1][kSQ] + 1 / sum_j K_ij

typedef float f16v __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// eight floats (two float4 at p0, p1) split exactly into truncated bf16
// pieces x = h + m + l, packed two per dword in k order
__device__ __forceinline__ void split3(const float* p0, const float* p1, u32x4& h, u32x4& m, u32x4& l) {
  const float4 a = *reinterpret_cast<const float4*>(p0), b = *reinterpret_cast<const float4*>(p1);
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    // the two residual subtractions of a pair as one v_pk_add_f32 each
    typedef unsigned int u2 __attribute__((ext_vector_type(2)));
    const f2 x = pk(v[2 * q], v[2 * q + 1]);
    const u2 xb = __builtin_bit_cast(u2, x);
    const f2 r1 = x - __builtin_bit_cast(f2, xb & 0xFFFF0000u);
    const u2 mb = __builtin_bit_cast(u2, r1) & 0xFFFF0000u;
    const u2 lb = __builtin_bit_cast(u2, r1 - __builtin_bit_cast(f2, mb));
    // high halves of (e0, e1) -> one dword, e0 in the low half
    h[q] = __builtin_amdgcn_perm(xb.y, xb.x, 0x07060302u);
    m[q] = __builtin_amdgcn_perm(mb.y, mb.x, 0x07060302u);
    l[q] = __builtin_amdgcn_perm(lb.y, lb.x, 0x07060302u);
  }
}

struct SiteArgs {
  const int* lanes;  // lane programs (trex_common.h)
  int64_t stride;    // ints per tree region
  const int8_t* leaves;
  const float* cost;
  int n_int, nl, L, tiles, B, Q;
  float a, bcoef;
  int hard_root;
  float* dp;          // [B][n_int][L][Q]
  float* site_score;  // [B][L] or null
  const float* dts;   // [B] or null
  float* marg;        // [B][n_int][L][Q] or null
  int8_t* anc;        // [B][n_int][L] or null
  double* part_tree;  // [B * tiles]
  double* part_dc;    // [Q * Q][B * tiles]
  const float* kg;    // K [kSQ][kSQ] and K^T (site_gate_write), zero-padded
  const float* ptab;  // cherry tables TM | TS (site_pair_tables), below K
  int cherry;         // one-wave kernel, 0: the CH = false variants (TREX_SITE_CHERRY=0, A/B; bitwise the same)
  float* srow;        // fused: s = K u of each computed internal child row, [B][n_int][L][Q]
  const int* flag;    // 1: this kernel handles the launch
  int n_slots;
};

// the arguments of a call, behind a gated wide_run (c.site_flag / c.site_kg),
// but the one-wave kernel's cherry (Args: SiteArgs, or the pair kernel's
// Site2Args)
template <class Args>
Args site_args(const SankoffCall& c, const int32_t* lanes, int lp_slots, int tiles) {
  Args A;
  fill_common(A, c, c.ni, c.L, tiles, (int64_t)c.B * tiles);
  A.lanes = lanes;
  A.stride = lp_tree_ints(c.ni);
  A.Q = c.Q;
  A.kg = c.site_kg;
  A.ptab = c.site_kg - kSiteTabBytes / 4;
  A.srow = c.phase == 3 ? c.site_srow : nullptr;
  A.flag = c.site_flag;
  A.n_slots = lp_slots;
  return A;
}

// diagnostic builds (TREX_SITE_TIMING / TREX_SITE2_TIMING, tools/site_times.py):
// lane 0 of every wave of the first 2048 workgroups stamps s_memtime at phase
// boundaries into the file's own table t[2048][waves][20]
#define SITE_STAMP_TO(t, j)                                                 \
  do {                                                                      \
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 2048 && (j) < 20)           \
      t[blockIdx.x][threadIdx.x >> 6][j] = __builtin_amdgcn_s_memtime();    \
  } while (0)

__device__ __forceinline__ void site_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ---- prologue pieces ----
// Only these two: the leaf message table's loop and the program / leaf-code
// staging stay spelled out in both kernels, because as functions (by
// reference, by value, in parts) they changed the one-wave kernels' machine
// code (PERFLOG).

// min C, by every wave for itself
__device__ __forceinline__ float site_cost_min(const float* cost, int Q, int lane) {
  float lmin = INFINITY;
  for (int e = lane; e < Q * Q; e += kWave) lmin = fminf(lmin, cost[e]);
  return uniform(wave_minf(lmin));
}

// sinv[i] = 1 / sum_j K_ij (0 for the padded states), by the first kSQ threads
__device__ __forceinline__ void site_row_sum_inv(const float* kg, int Q, float* sinv) {
  if (threadIdx.x < kSQ) {
    const int i = threadIdx.x;
    float sk = 0.0f;
    for (int j = 0; j < Q; ++j) sk += kg[i * kSQ + j];
    sinv[i] = i < Q ? __builtin_amdgcn_rcpf(sk) : 0.0f;
  }
}

}  // namespace
}  // namespace trex
