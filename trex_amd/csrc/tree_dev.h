// What the tree-cost translation units share (tree.hip, tree_gram.hip,
// tree_mf.hip, tree_opt.hip): vector types, a few device helpers, the step
// state and the host functions that cross files.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdlib>

#include "sankoff_dev.h"
#include "trex_common.h"

namespace trex {

// Host functions defined once and called across files (library-internal:
// hidden, so the exported symbols are the C ABI's only).
#define TREX_LOCAL __attribute__((visibility("hidden")))
// tree.hip: blocks of `per` for n items, at most cap
TREX_LOCAL int grid_for(int64_t n, int per = 256, int cap = 8192);
// tree.hip: the power of two s with max_abs * s <= 2^14 (f16 split headroom)
TREX_LOCAL float split_scale(float max_abs);
// tree_gram.hip: gram()'s split-K partial buffer, the head of the workspace
TREX_LOCAL int64_t part_bytes(int N, int64_t K);
// tree_gram.hip: G = X Y^T.  x3_max > 0: f16x3 split products with operands
// bounded by x3_max; pre: X pre-split (split_x3_group layout); lzs / codes:
// leaf strips with a zero lo plane / read as their code bytes
TREX_LOCAL int gram(const float* X, const float* Y, int N, int64_t K, int symmetric, float* G,
                    float* part, hipStream_t st, int t0 = 0, float x3_max = 0.0f,
                    bool pre = false, int lzs = 0, const uint8_t* codes = nullptr);
// tree_mf.hip: out = M[row0 : row0 + nrows] S on the one-wave-per-tile f32
// kernel (any K)
TREX_LOCAL void launch_mf2(const float* M, const float* S, int N, int K, int row0, int nrows,
                           float* out, hipStream_t st);

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float fv4 __attribute__((ext_vector_type(4)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

// a run-time switch (TREX_GRAM, TREX_MF, TREX_GRAM_LZ), read per call: tests
// flip them inside one process
inline int env_int(const char* name, int unset) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) : unset;
}

__device__ __forceinline__ double block_sum_256(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// workgroup barrier for LDS hand-over only: waits for this wave's LDS ops
// (lgkmcnt) but NOT for its outstanding global loads -- __syncthreads()'s
// fence would drain vmcnt and so the register prefetch of the next chunk
// at every barrier
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ---- f16x3 split products (X3 variants) --------------------------------
// x*s = hi + lo with hi = f16(x*s), lo = f16(x*s - hi): 22 significant bits;
// x*y ~ hi_x hi_y + hi_x lo_y + lo_x hi_y (lo_x lo_y, ~2^-22 relative, and
// the split residuals dropped) on v_mfma_f32_32x32x16_f16 with f32
// accumulation: 3 f16 MFMAs (96 cycles/SIMD) replace 8 f32 ones (512) per
// 32x32x16 block.  The power-of-two operand scales keep |x*s| <= 2^14 (no
// f16 overflow) and lo out of the f16 subnormal range; the result is scaled
// back exactly.  Error per product <~ 1e-6 relative, random in sign: the
// tests hold these GEMMs to the same rtol 1e-5 vs fp64 as the f32 path.
// (The hi / lo split is spelled out at each of its seven sites -- here twice,
// g3_stage, the MF kernels' stages: routing them through one helper changed
// the machine code of 11 kernels, PERFLOG.)
__device__ __forceinline__ void split_h8(const float (&x)[8], float scale, h8& hi, h8& lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = x[j] * scale;
    const _Float16 h = (_Float16)v;
    hi[j] = h;
    lo[j] = (_Float16)(v - (float)h);
  }
}
__device__ __forceinline__ f32x16 mfma_x3(const h8& ah, const h8& al, const h8& bh, const h8& bl,
                                          f32x16 acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
}

// f16x3 operand pre-split (x3p entry points, trex_tree_split_x3): every
// group of 4 consecutive f32 values x * s is stored as 16 bytes -- the four
// f16 hi parts, then the four f16 lo parts -- so a 16-B load of the
// pre-split operand lands at the same byte offset as the f32 one and the
// kernels stage it into LDS without the split arithmetic
__device__ __forceinline__ u32x4 split_x3_group(float x0, float x1, float x2, float x3, float s) {
  const float v[4] = {x0 * s, x1 * s, x2 * s, x3 * s};
  h4 hi, lo;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    hi[j] = (_Float16)v[j];
    lo[j] = (_Float16)(v[j] - (float)hi[j]);
  }
  const uint2 a = __builtin_bit_cast(uint2, hi), b = __builtin_bit_cast(uint2, lo);
  return (u32x4){a.x, a.y, b.x, b.y};
}

// Device step state of a graph-capturable optimisation loop
// (trex_step_advance): the 1-based step count and what the step's kernels
// derive from it -- Adam's bias corrections and the annealing schedule's
// temperature of this step and the next -- so a captured step replays with
// the right values (the reference's lax.fori_loop / scan carry,
// src/trex/evals/benchmark.py:167-200).  A null state pointer: host values.
struct StepState {
  int count;
  float bc1, bc2, T, Tn;
  float pad[3];
};
static_assert(sizeof(StepState) == 32, "step state layout");

}  // namespace
}  // namespace trex
