// libtrexhip.so -- the tree-cost Gram G = X Y^T (tree.hip has the map of the
// tree-cost files).  Kernels: v1 / v2 (one wave per 64x64 tile, operands from
// L2: any shape), v3 (LDS-staged f16x3, two waves per SIMD: the x3 default),
// v5 (one wave per SIMD, pipelined fragment reads: the f32 default; its
// W = 8 arm is "v6").  gram() holds the one launch table.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "tree_dev.h"

namespace trex {
namespace {

// ---------------------------------------------------------------------------
// a9 Gram G = X Y^T on MFMA f32 (X, Y: [N][K] row-major).  One wave computes
// a 64x64 tile (2x2 32x32 accumulators) over one K slice.  Lane l (row
// r = l&31, half h = l>>5) loads 16 consecutive k of its row per fragment;
// MFMA t then covers k = kb + t and kb + 16 + t on the two halves (the k
// permutation is the same for X and Y, so the dot products are exact).
// Blocks are grouped so that one XCD (blockIdx % 8) walks the tiles of one
// K slice while that slice is L2-resident.
// ---------------------------------------------------------------------------
// 16 consecutive k of one row (row stride K), zero past kend / nrows
__device__ __forceinline__ void load_frag16(const float* __restrict__ base, int row, int nrows,
                                            int K, int k0, int kend, float (&o)[16]) {
  if (row < nrows && k0 + 16 <= kend && (K & 3) == 0) {
    const float4* p = reinterpret_cast<const float4*>(base + (size_t)row * K + k0);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float4 v = p[t];
      o[4 * t] = v.x; o[4 * t + 1] = v.y; o[4 * t + 2] = v.z; o[4 * t + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int t = 0; t < 16; ++t)
      o[t] = (row < nrows && k0 + t < kend) ? base[(size_t)row * K + k0 + t] : 0.0f;
  }
}

// pair -> (ti, tj).  symmetric: the upper triangle (ti <= tj) row-major,
// minus the tiles with both ti, tj < t0 (a cached constant block, e.g. the
// fixed leaf x leaf Gram of the C5 loop)
__host__ __device__ __forceinline__ int sym_row_len(int a, int ntile, int t0) {
  return ntile - (a > t0 ? a : t0);
}
__device__ __forceinline__ void pair_tiles(int pair, int ntile, int symmetric, int t0, int* ti,
                                           int* tj) {
  if (symmetric) {
    int a = 0, rem = pair;
    while (rem >= sym_row_len(a, ntile, t0)) { rem -= sym_row_len(a, ntile, t0); ++a; }
    *ti = a;
    *tj = (a > t0 ? a : t0) + rem;
  } else {
    *ti = pair / ntile;
    *tj = pair % ntile;
  }
}

__global__ __launch_bounds__(kWave) void gram_kernel(const float* __restrict__ X,
                                                    const float* __restrict__ Y, int N, int K,
                                                    int ntile, int npairs, int symmetric, int t0,
                                                    int ksplit, int kslice,
                                                    float* __restrict__ part) {
  const int b = blockIdx.x;
  const int xcd = b & 7, m = b >> 3;
  const int split = (m / npairs) * 8 + xcd;
  const int pair = m % npairs;
  if (split >= ksplit) return;
  int ti, tj;
  pair_tiles(pair, ntile, symmetric, t0, &ti, &tj);
  const int lane = threadIdx.x;
  const int r = lane & 31, h = lane >> 5;
  const int k_lo = split * kslice, k_hi = min(K, k_lo + kslice);
  f32x16 acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) acc[u][v] = (f32x16){};
  for (int kb = k_lo; kb < k_hi; kb += 32) {
    float xa[2][16], yb[2][16];
#pragma unroll
    for (int u = 0; u < 2; ++u) load_frag16(X, ti * 64 + u * 32 + r, N, K, kb + 16 * h, k_hi, xa[u]);
#pragma unroll
    for (int v = 0; v < 2; ++v) load_frag16(Y, tj * 64 + v * 32 + r, N, K, kb + 16 * h, k_hi, yb[v]);
#pragma unroll
    for (int t = 0; t < 16; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v)
          acc[u][v] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[u][t], yb[v][t], acc[u][v], 0, 0, 0);
  }
  // partial tile [split][pair][64][64]
  float* out = part + ((size_t)split * npairs + pair) * 64 * 64;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
        out[(u * 32 + row) * 64 + v * 32 + r] = acc[u][v][q];
      }
}

// v2 Gram: k step 16 per fragment, the next step's fragments requested
// before this step's MFMAs (ping-pong registers, loop unrolled by two so
// nothing is copied).  Lane (r, h) loads X[row][kb + 8h .. kb + 8h + 8)
// (two float4); MFMA t covers k = kb + t (h = 0) and kb + 8 + t (h = 1).
// Loads are unconditional (clamped row, zero select) so every path issues
// the same VMEM ops.  Needs K % 16 == 0 and kslice % 32 == 0.
__device__ __forceinline__ void load_rows8(const float* __restrict__ base, int row0, int nrows,
                                           int K, int k0, float (&o)[2][8]) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int row = row0 + u * 32;
    const bool ok = row < nrows;
    const float4* p = reinterpret_cast<const float4*>(base + (size_t)(ok ? row : 0) * K + k0);
    const float4 a = p[0], b = p[1];
    o[u][0] = ok ? a.x : 0.0f; o[u][1] = ok ? a.y : 0.0f; o[u][2] = ok ? a.z : 0.0f;
    o[u][3] = ok ? a.w : 0.0f; o[u][4] = ok ? b.x : 0.0f; o[u][5] = ok ? b.y : 0.0f;
    o[u][6] = ok ? b.z : 0.0f; o[u][7] = ok ? b.w : 0.0f;
  }
}

// X3: f16x3 split products; sx, sy operand scales, out scaled by 1/(sx sy)
template <bool X3>
__global__ __launch_bounds__(kWave) void gram_kernel2(const float* __restrict__ X,
                                                     const float* __restrict__ Y, int N, int K,
                                                     int ntile, int npairs, int symmetric, int t0,
                                                     int ksplit, int kslice,
                                                     float* __restrict__ part, float sx = 1.0f,
                                                     float sy = 1.0f) {
  const int b = blockIdx.x;
  const int xcd = b & 7, m = b >> 3;
  const int split = (m / npairs) * 8 + xcd;
  const int pair = m % npairs;
  if (split >= ksplit) return;
  int ti, tj;
  pair_tiles(pair, ntile, symmetric, t0, &ti, &tj);
  const int lane = threadIdx.x;
  const int r = lane & 31, h = lane >> 5;
  const int k_lo = split * kslice, k_hi = min(K, k_lo + kslice);
  f32x16 acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) acc[u][v] = (f32x16){};
  const int xr = ti * 64 + r, yr = tj * 64 + r;
  auto fetch = [&](int kb, float (&xa)[2][8], float (&yb)[2][8]) {
    const int k0 = min(kb, K - 16) + 8 * h;  // past k_hi: a valid address, product masked below
    load_rows8(X, xr, N, K, k0, xa);
    load_rows8(Y, yr, N, K, k0, yb);
  };
  auto compute = [&](int kb, float (&xa)[2][8], float (&yb)[2][8]) {
    if (kb >= k_hi) return;
    if constexpr (X3) {
      // lane (r, h) holds A[row r][k = 8h + j] and B[k = 8h + j][col r]: the
      // 32x32x16 f16 fragments are exactly the loaded 8-float runs
      h8 xh[2], xl[2], yh[2], yl[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) split_h8(xa[u], sx, xh[u], xl[u]);
#pragma unroll
      for (int v = 0; v < 2; ++v) split_h8(yb[v], sy, yh[v], yl[v]);
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = mfma_x3(xh[u], xl[u], yh[v], yl[v], acc[u][v]);
    } else {
#pragma unroll
      for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int v = 0; v < 2; ++v)
            acc[u][v] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[u][t], yb[v][t], acc[u][v], 0, 0, 0);
    }
  };
  float xa0[2][8], yb0[2][8], xa1[2][8], yb1[2][8];
  fetch(k_lo, xa0, yb0);
  for (int kb = k_lo; kb < k_hi; kb += 32) {
    fetch(kb + 16, xa1, yb1);
    compute(kb, xa0, yb0);
    fetch(kb + 32, xa0, yb0);
    compute(kb + 16, xa1, yb1);
  }
  const float unscale = X3 ? 1.0f / (sx * sy) : 1.0f;
  float* out = part + ((size_t)split * npairs + pair) * 64 * 64;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
        out[(u * 32 + row) * 64 + v * 32 + r] = acc[u][v][q] * unscale;
      }
}

// G[i][j] = sum over splits (fixed order, fp64); symmetric tiles mirrored
__global__ __launch_bounds__(256) void gram_reduce_kernel(const float* __restrict__ part, int N,
                                                         int ntile, int npairs, int ksplit,
                                                         int symmetric, int t0,
                                                         float* __restrict__ G) {
  const size_t total = (size_t)npairs * 4096;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
    const int pair = (int)(t / 4096);
    const int e = (int)(t % 4096);
    int ti, tj;
    pair_tiles(pair, ntile, symmetric, t0, &ti, &tj);
    double s = 0.0;
    for (int sp = 0; sp < ksplit; ++sp) s += (double)part[((size_t)sp * npairs + pair) * 4096 + e];
    const int i = ti * 64 + e / 64, j = tj * 64 + e % 64;
    // a diagonal tile holds both (i, j) and (j, i): only i <= j writes the
    // pair, or two threads would race on it with differently rounded sums
    if (i < N && j < N && (!symmetric || ti != tj || i <= j)) {
      G[(size_t)i * N + j] = (float)s;
      if (symmetric) G[(size_t)j * N + i] = (float)s;
    }
  }
}

// ---- v3 Gram: LDS-staged K chunks, one workgroup per CU -------------------
// Symmetric G = S S^T (f16x3 split products) over the needed 32x32 tiles:
// the upper triangle minus the cached leaf x leaf block (tiles with both
// strips < t0s), enumerated row-major like pair_tiles.  A workgroup is 8
// waves, two per SIMD (256 registers each, no spills): a wave owns up to 13
// tiles (208 accumulator registers); a workgroup owns up to 104 tiles (a
// "group"; more tiles -> more groups; C5's 100 tiles are one) and a
// contiguous range of 16-wide K chunks (its split), one workgroup per CU.
// Per chunk all N <= 512 rows are loaded ONCE from HBM (one dwordx4 per
// thread per 128 rows, issued a chunk ahead into
// registers), split into f16 hi / lo planes in LDS (double-buffered, row
// stride 80 B: hi k0..15 | lo k0..15 | pad), and every wave feeds its
// tiles' 32x32x16 MFMAs from LDS fragments (the A fragment re-read only when
// the tile row strip changes).  The v2 kernel instead re-read each row once
// per 64x64 tile pair from L2 with one wave per pair: load-bound.
// Partials [split][tile][32][32] (scaled back) reduce in a fixed order.
constexpr int kG3Rows = 512;
constexpr int kG3Stride = 80;
constexpr int kG3Tiles = 13;
constexpr int kG3Waves = 8;
constexpr int kG3Rows4 = kG3Waves * 64 / 4;  // rows per load pass (128)
constexpr int kG3Buf = kG3Rows * kG3Stride;
constexpr int kG3Lds = 2 * kG3Buf;

template <bool PRE = false>
__device__ __forceinline__ void g3_stage(unsigned char* buf, int row, int sub, const u32x4& w,
                                         float sc) {
  if constexpr (PRE) {
    *reinterpret_cast<uint2*>(buf + row * kG3Stride + sub * 8) = uint2{w.x, w.y};
    *reinterpret_cast<uint2*>(buf + row * kG3Stride + 32 + sub * 8) = uint2{w.z, w.w};
    return;
  }
  const float v[4] = {__uint_as_float(w.x) * sc, __uint_as_float(w.y) * sc,
                      __uint_as_float(w.z) * sc, __uint_as_float(w.w) * sc};
  h4 hi, lo;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    hi[j] = (_Float16)v[j];
    lo[j] = (_Float16)(v[j] - (float)hi[j]);
  }
  *reinterpret_cast<h4*>(buf + row * kG3Stride + sub * 8) = hi;
  *reinterpret_cast<h4*>(buf + row * kG3Stride + 32 + sub * 8) = lo;
}

// NCP (PRE only): rows [0, 128 NCP) -- the first NCP row passes -- are exact
// one-hot leaf rows read as their code bytes (codes, trex_tree_leaf_codes;
// one byte per site instead of a 16-B pre-split piece) and expanded into
// the same f16 image (hi = one-hot x sc, lo = 0): bitwise the pre-split rows.
// The pass split is compile-time: a runtime per-row choice spilled (11-16
// VGPRs) and cost the whole kernel 1.7x
template <bool PRE = false, int NCP = 0>  // PRE: S pre-split (split_x3_group layout)
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void gram_kernel3(
    const float* __restrict__ S, int N, int K, int ns, int t0s, int ntiles, int ngroups,
    int ksplit, int nchunks, float sc, float* __restrict__ part, int lzs = 0,
    const uint8_t* __restrict__ codes = nullptr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds3[];
  const int g = blockIdx.x % ngroups;
  const int split = blockIdx.x / ngroups;
  const int c_lo = (int)((int64_t)split * nchunks / ksplit);
  const int c_hi = (int)((int64_t)(split + 1) * nchunks / ksplit);
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 31, h = lane >> 5;
  const int tb = (g * kG3Waves + wave) * kG3Tiles;
  const int nt = max(0, min(kG3Tiles, ntiles - tb));
  // first tile's strips; tiles past the wave's range (t >= nt) run on
  // whatever strips follow (clamped to ns - 1) and are not written: every
  // wave issues the same unconditional MFMA stream.  (Spreading the leaf
  // strips' 2-MFMA tiles evenly over the SIMDs measured no gain, PERFLOG.)
  int a0, b0;
  pair_tiles(min(tb, ntiles - 1), ns, 1, t0s, &a0, &b0);

  f32x16 acc[kG3Tiles];
#pragma unroll
  for (int t = 0; t < kG3Tiles; ++t) acc[t] = (f32x16){};

  // loads: thread (rb = tid / 4, sub = tid % 4) fetches S[rb + 128 i][k0 + 4 sub .. + 4);
  // rows past N read out of bounds (0)
  const rsrc_t rs = make_rsrc(S, (uint32_t)((size_t)N * K * 4));
  const int sub = tid & 3, rb = tid >> 2;
  constexpr int kRowsPerPass = kG3Waves * kWave / 4;
  static_assert(NCP == 0 || PRE, "code rows need the pre-split image");
  u32x4 pf[kG3Rows / kRowsPerPass - NCP];
  uint32_t pcode[NCP > 0 ? NCP : 1];
  const rsrc_t rcd = make_rsrc(codes, (uint32_t)((size_t)kRowsPerPass * NCP * (K / 4)));
  auto gload = [&](int c) {
#pragma unroll
    for (int i = 0; i < kG3Rows / kRowsPerPass; ++i) {
      const int vo = ((rb + kRowsPerPass * i) * K + 4 * sub) * 4;  // code byte: vo / 16
      if (i < NCP)
        pcode[i < NCP ? i : 0] = __builtin_amdgcn_raw_buffer_load_b8(rcd, vo >> 4, c * 4, 0);
      else
        pf[i - NCP] = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, c * 64, 0);
    }
  };
  const uint32_t hb = (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)sc);  // one-hot 1 x sc
  // K % 16 != 0 (K % 4 == 0): the last chunk's columns past K hold the next
  // row's first values (or read out of bounds: 0); staged as zeros, they add
  // nothing to any product
  auto stage = [&](unsigned char* buf, int c) {
    const bool kv = 16 * c + 4 * sub < K;
#pragma unroll
    for (int i = 0; i < kG3Rows / kRowsPerPass; ++i)
    {
      const int row = rb + kRowsPerPass * i;
      if (i < NCP) {
        const uint32_t code = kv ? (pcode[i < NCP ? i : 0] & 0xFFu) : 0xFFu;
        const u32x4 w = {(code == 0 ? hb : 0u) | ((code == 1 ? hb : 0u) << 16),
                         (code == 2 ? hb : 0u) | ((code == 3 ? hb : 0u) << 16), 0u, 0u};
        g3_stage<true>(buf, row, sub, w, sc);
      } else {
        g3_stage<PRE>(buf, row, sub, kv ? pf[i - NCP] : (u32x4){0u, 0u, 0u, 0u}, sc);
      }
    }
  };
  const int lofs = r * kG3Stride + 16 * h;
  auto compute = [&](const unsigned char* buf) {
    int a = a0, b = b0, ap = -1;
    h8 ah, al;
    // B fragments one tile ahead: tile t + 1's reads are issued before tile
    // t's MFMAs (the A fragment only when the row strip changes: a wave's
    // 13 tiles span 2-3 strips; LDS read bytes per chunk 416 -> ~240 KB per CU)
    h8 bh = *reinterpret_cast<const h8*>(buf + b * (32 * kG3Stride) + lofs);
    h8 bl = *reinterpret_cast<const h8*>(buf + b * (32 * kG3Stride) + lofs + 32);
#pragma unroll
    for (int t = 0; t < kG3Tiles; ++t) {
      // strips a < lzs: exact one-hot leaf rows, whose lo plane is zero
      const bool zlo = a < lzs;
      if (a != ap) {
        const unsigned char* pa = buf + a * (32 * kG3Stride) + lofs;
        ah = *reinterpret_cast<const h8*>(pa);
        al = *reinterpret_cast<const h8*>(pa + 32);
        ap = a;
      }
      const bool wrap = b + 1 >= ns;
      const int an = wrap ? min(a + 1, ns - 1) : a;
      const int bn = wrap ? (an > t0s ? an : t0s) : b + 1;
      h8 bhn = bh, bln = bl;
      if (t + 1 < kG3Tiles) {
        const unsigned char* pb = buf + bn * (32 * kG3Stride) + lofs;
        bhn = *reinterpret_cast<const h8*>(pb);
        bln = *reinterpret_cast<const h8*>(pb + 32);
      }
      __builtin_amdgcn_sched_barrier(0);  // keep the prefetch reads above the MFMAs
      // a zero lo plane adds exact zeros: its MFMA is skipped (bitwise)
      if (!zlo) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[t], 0, 0, 0);
      bh = bhn;
      bl = bln;
      a = an;
      b = bn;
    }
  };

  if (c_lo < c_hi) {
    gload(c_lo);
    stage(lds3, c_lo);
    if (c_lo + 1 < c_hi) gload(c_lo + 1);
  }
  lds_barrier();
  for (int c = c_lo; c < c_hi; ++c) {
    unsigned char* cb = lds3 + ((c - c_lo) & 1) * kG3Buf;
    unsigned char* nb = lds3 + (((c - c_lo) & 1) ^ 1) * kG3Buf;
    compute(cb);
    if (c + 1 < c_hi) {
      stage(nb, c + 1);
      if (c + 2 < c_hi) gload(c + 2);
    }
    lds_barrier();
  }

  const float unscale = 1.0f / (sc * sc);
#pragma unroll
  for (int t = 0; t < kG3Tiles; ++t) {
    if (t < nt) {
      float* out = part + ((size_t)split * ntiles + tb + t) * 1024;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
        out[row * 32 + r] = acc[t][q] * unscale;
      }
    }
  }
}

// G[i][j] = G[j][i] = sum over splits of the v3 partials, fp64 in a fixed
// association: thread (e, q) of a block (64 elements x 4 quarters) sums the
// splits sp = q, q + 4, ... in order (4 independent loads in flight), then
// the four quarter sums add in q order.  One wave reads 256 contiguous bytes
// per split; the grid has ntiles * 16 waves (the serial one-thread-per-
// element loop kept too few loads in flight: 1.4 TB/s).
__global__ __launch_bounds__(256) void gram3_reduce_kernel(const float* __restrict__ part, int N,
                                                          int ns, int t0s, int ntiles,
                                                          int ksplit, float* __restrict__ G) {
  __shared__ double qs[4][64];
  const int el = threadIdx.x & 63, q = threadIdx.x >> 6;
  const size_t t = (size_t)blockIdx.x * 64 + el;  // element index, < ntiles * 1024
  const size_t stride = (size_t)ntiles * 1024;
  const float* src = part + t;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int sp = q;
  for (; sp + 12 < ksplit; sp += 16) {
    s0 += (double)src[(size_t)sp * stride];
    s1 += (double)src[(size_t)(sp + 4) * stride];
    s2 += (double)src[(size_t)(sp + 8) * stride];
    s3 += (double)src[(size_t)(sp + 12) * stride];
  }
  for (; sp < ksplit; sp += 4) s0 += (double)src[(size_t)sp * stride];
  qs[q][el] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (q != 0) return;
  const double s = ((qs[0][el] + qs[1][el]) + qs[2][el]) + qs[3][el];
  const int tile = (int)(t >> 10);
  const int e = (int)(t & 1023);
  int si, sj;
  pair_tiles(tile, ns, 1, t0s, &si, &sj);
  const int i = si * 32 + (e >> 5), j = sj * 32 + (e & 31);
  // diagonal tiles: only i <= j writes the mirrored pair (no write race)
  if (i < N && j < N && (si != sj || i <= j)) {
    G[(size_t)i * N + j] = (float)s;
    G[(size_t)j * N + i] = (float)s;
  }
}

// ---- v5 Gram: one wave per SIMD, software-pipelined fragment reads ---------
// v3's tile enumeration and staging, re-shaped for the MFMA pipe (v3 lost
// ~60 % of it: every tile's fragments were read right before its MFMAs behind
// an lgkmcnt(0), and the A-fragment reuse branch split the loop into one
// basic block per tile).  Here a workgroup is 4 waves (one per SIMD, up to
// 512 registers: the accumulators live in AGPRs); a wave owns T <= 16
// consecutive tiles and reads tile t + 1's A / B fragments (4 ds_read_b128)
// while tile t's three MFMAs run -- no branch anywhere in the chunk body, so
// the per-row f16 staging of the next chunk and the global loads of the
// chunk after it are interleaved between the MFMAs (row i of the stage after
// tile i; raw rows one chunk ahead in registers).
// A workgroup holds at most 64 tiles, so C5's 100 tiles take two groups; the
// two groups of a K split sit on the same XCD (blockIdx % 8) and run at the
// same pace, so the second read of each chunk is an L2 hit.
// X3 = false: the exact f32 Gram on v_mfma_f32_32x32x2_f32 -- rows staged as
// f32 (the same 80-B row stride), a lane's 8 k of a fragment (k = 8h .. 8h +
// 7) read as two float4 and fed to 8 MFMAs (MFMA t covers k = t and 8 + t on
// the two lane halves: the same permutation for both operands).
constexpr int kG5Waves = 4;
constexpr int kG5MaxTiles = 16;

// W = 8 (two waves per SIMD, T <= 8 tiles each: 128 accumulator registers)
// is the x3 variant under test (TREX_GRAM=6)
template <int T, bool X3, int W = kG5Waves>
__global__ __launch_bounds__(W * 64) __attribute__((amdgpu_waves_per_eu(W / 4, W / 4))) void gram_kernel5(
    const float* __restrict__ S, int N, int K, int ns, int t0s, int ntiles, int ngroups,
    int ksplit, int nchunks, float sc, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds5[];
  const int xcd = blockIdx.x & 7, m = blockIdx.x >> 3;
  const int g = m % ngroups;
  const int split = (m / ngroups) * 8 + xcd;
  if (split >= ksplit) return;
  const int c_lo = (int)((int64_t)split * nchunks / ksplit);
  const int c_hi = (int)((int64_t)(split + 1) * nchunks / ksplit);
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 31, h = lane >> 5;
  const int tb = (g * W + wave) * T;
  const int nt = max(0, min(T, ntiles - tb));
  // per-slot strip byte offsets (wave-uniform); slots past the wave's range
  // repeat the last strips and are not stored
  int offA[T], offB[T];
  {
    int a, b;
    pair_tiles(min(tb, ntiles - 1), ns, 1, t0s, &a, &b);
#pragma unroll
    for (int t = 0; t < T; ++t) {
      offA[t] = a * (32 * kG3Stride);
      offB[t] = b * (32 * kG3Stride);
      const bool wrap = b + 1 >= ns;
      const int an = wrap ? min(a + 1, ns - 1) : a;
      b = wrap ? (an > t0s ? an : t0s) : b + 1;
      a = an;
    }
  }

  f32x16 acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = (f32x16){};

  const rsrc_t rs = make_rsrc(S, (uint32_t)((size_t)N * K * 4));
  const int sub = tid & 3, rb = tid >> 2;
  constexpr int kRowsPerPass = W * kWave / 4;  // 64 (W = 4) / 128 (W = 8)
  constexpr int kPasses = kG3Rows / kRowsPerPass;     // 8
  u32x4 pf[kPasses];
  auto gload1 = [&](int i, int c) {
    pf[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, ((rb + kRowsPerPass * i) * K + 4 * sub) * 4,
                                                  __builtin_amdgcn_readfirstlane(c * 64), 0);
  };
  auto stage1 = [&](unsigned char* buf, int i, int c) {
    const bool kv = 16 * c + 4 * sub < K;
    const u32x4 w = kv ? pf[i] : (u32x4){0u, 0u, 0u, 0u};
    if constexpr (X3)
      g3_stage(buf, rb + kRowsPerPass * i, sub, w, sc);
    else
      *reinterpret_cast<u32x4*>(buf + (rb + kRowsPerPass * i) * kG3Stride + 16 * sub) = w;
  };
  const int lofs = r * kG3Stride + (X3 ? 16 : 32) * h;
  h8 fa[2][2], fb[2][2];
  f32x8 ga[2], gb[2];
  auto rd = [&](const unsigned char* cb, int t, int s) {
    const unsigned char* pa = cb + offA[t] + lofs;
    const unsigned char* pb = cb + offB[t] + lofs;
    if constexpr (X3) {
      fa[s][0] = *reinterpret_cast<const h8*>(pa);
      fa[s][1] = *reinterpret_cast<const h8*>(pa + 32);
      fb[s][0] = *reinterpret_cast<const h8*>(pb);
      fb[s][1] = *reinterpret_cast<const h8*>(pb + 32);
    } else {
      ga[s] = *reinterpret_cast<const f32x8*>(pa);
      gb[s] = *reinterpret_cast<const f32x8*>(pb);
    }
  };

  if (c_lo < c_hi) {
#pragma unroll
    for (int i = 0; i < kPasses; ++i) gload1(i, c_lo);
#pragma unroll
    for (int i = 0; i < kPasses; ++i) {
      stage1(lds5, i, c_lo);
      gload1(i, c_lo + 1);
    }
  }
  lds_barrier();
  // chunk c: MFMAs on buf[(c - c_lo) & 1]; stage chunk c + 1 (in pf) into
  // the other buffer and refill pf with chunk c + 2.  Past the split's last
  // chunk the stage and loads run on (ignored) neighbouring data: the body
  // stays branch-free.
  for (int c = c_lo; c < c_hi; ++c) {
    const int odd = (c - c_lo) & 1;
    const unsigned char* cb = lds5 + odd * kG3Buf;
    unsigned char* nb = lds5 + (odd ^ 1) * kG3Buf;
    rd(cb, 0, 0);
#pragma unroll
    for (int t = 0; t < T; ++t) {
      if (t + 1 < T) rd(cb, t + 1, (t + 1) & 1);
      if constexpr (X3) {
        acc[t] = mfma_x3(fa[t & 1][0], fa[t & 1][1], fb[t & 1][0], fb[t & 1][1], acc[t]);
      } else {
#pragma unroll
        for (int q = 0; q < 8; ++q)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[t & 1][q], gb[t & 1][q], acc[t], 0, 0, 0);
      }
      if (t < kPasses) {
        stage1(nb, t, c + 1);
        gload1(t, c + 2);
      }
    }
#pragma unroll
    for (int i = T; i < kPasses; ++i) {
      stage1(nb, i, c + 1);
      gload1(i, c + 2);
    }
    lds_barrier();
  }

  const float unscale = 1.0f / (sc * sc);
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if (t < nt) {
      float* out = part + ((size_t)split * ntiles + tb + t) * 1024;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
        out[row * 32 + r] = acc[t][q] * unscale;
      }
    }
  }
}

// G[i][j] = G[j][i] for i < row0 <= j: after a site-sharded all-reduce of
// the rows [row0, N) only, the leaf rows' ancestor columns take the reduced
// values (the leaf x leaf block [0, row0)^2 is a cached global constant)
__global__ __launch_bounds__(256) void gram_mirror_kernel(float* __restrict__ G, int N, int row0) {
  const int64_t n = (int64_t)row0 * (N - row0);
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
    const int i = (int)(t / (N - row0)), j = row0 + (int)(t % (N - row0));
    G[(size_t)i * N + j] = G[(size_t)j * N + i];
  }
}

// x3p operands: rows x cols of X (row stride ldx) -> split_x3_group layout,
// ldo f32-equivalent columns per row (groups past cols are zero)
__global__ __launch_bounds__(256) void split_x3_kernel(const float* __restrict__ X, int rows,
                                                      int cols, int ldx, float s,
                                                      u32x4* __restrict__ out, int ldo) {
  const int G = ldo / 4;
  const int64_t n = (int64_t)rows * G;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
    const int row = (int)(t / G), c = 4 * (int)(t % G);
    const float* x = X + (size_t)row * ldx;
    out[t] = split_x3_group(c < cols ? x[c] : 0.0f, c + 1 < cols ? x[c + 1] : 0.0f,
                            c + 2 < cols ? x[c + 2] : 0.0f, c + 3 < cols ? x[c + 3] : 0.0f, s);
  }
}

struct GramPlan {
  int ntile, npairs, ksplit, kslice;
};
GramPlan gram_plan(int N, int64_t K, bool symmetric = false, int t0 = 0) {
  GramPlan g;
  g.ntile = (N + 63) / 64;
  // workspace is sized for the full (non-symmetric) tile set
  if (symmetric) {
    g.npairs = 0;
    for (int a = 0; a < g.ntile; ++a) g.npairs += sym_row_len(a, g.ntile, t0);
  } else {
    g.npairs = g.ntile * g.ntile;
  }
  // enough waves to fill 256 CUs several times; slices multiple of 32
  int ks = (int)std::max<int64_t>(1, std::min<int64_t>(256, (4096 + g.npairs - 1) / g.npairs));
  ks = (ks + 7) / 8 * 8;
  int64_t slice = (K + ks - 1) / ks;
  slice = (slice + 31) / 32 * 32;
  g.kslice = (int)std::max<int64_t>(32, slice);
  g.ksplit = (int)((K + g.kslice - 1) / g.kslice);
  return g;
}

// v3 plan (symmetric, N <= 512, K % 4 == 0: 16-B aligned rows; a ragged
// last 16-column chunk is zero-masked in the kernel): 32-row strips, tiles per
// group of 8 waves x 13, about one workgroup per CU
struct Gram3Plan {
  int ns, t0s, ntiles, ngroups, ksplit, nchunks;
};
Gram3Plan gram3_plan(int N, int64_t K, int t0s) {
  Gram3Plan g;
  g.ns = (N + 31) / 32;
  g.t0s = t0s;
  g.ntiles = 0;
  for (int a = 0; a < g.ns; ++a) g.ntiles += sym_row_len(a, g.ns, t0s);
  g.ngroups = std::max(1, (g.ntiles + kG3Waves * kG3Tiles - 1) / (kG3Waves * kG3Tiles));
  g.nchunks = (int)((K + 15) / 16);
  g.ksplit = std::max(1, std::min(g.nchunks, std::max(1, 256 / g.ngroups)));
  return g;
}
// v5: ngroups = ceil(ntiles / 64), T = tiles per wave; ksplit a multiple of
// 8 (the XCD pairing of a split's groups), about one workgroup per CU
Gram3Plan gram5_plan(int N, int64_t K, int t0s, int* T, int W = kG5Waves) {
  Gram3Plan g = gram3_plan(N, K, t0s);
  const int maxt = W == 8 ? 8 : kG5MaxTiles;
  g.ngroups = std::max(1, (g.ntiles + W * maxt - 1) / (W * maxt));
  *T = std::max(1, (g.ntiles + W * g.ngroups - 1) / (W * g.ngroups));
  int ks = std::max(1, 256 / g.ngroups);
  ks = std::max(8, ks / 8 * 8);
  g.ksplit = std::max(1, std::min(g.nchunks, ks));
  return g;
}
// kernel version per precision: f32 -> v5 (one wave per SIMD: the 64-cycle
// f32 MFMAs fill the pipe; 587 -> 397 us at C5), x3 -> v3 (two waves per
// SIMD: the f16 MFMA chains need the second wave; v5 measured 231 vs 152
// us).  TREX_GRAM=3 / 5 forces one version for both (A/B); 6: v5 with the
// x3 arm at W = 8 (measured, not adopted: PERFLOG).
int gram_version(bool x3) {
  const int e = env_int("TREX_GRAM", 0);
  return (e == 3 || e == 5 || e == 6) ? e : (x3 ? 3 : 5);
}
bool gram3_ok(int N, int64_t K) { return N <= kG3Rows && K % 4 == 0 && (int64_t)N * K * 4 < 0x7FFFFFF0LL; }

// ---- the launch table of the LDS-staged kernels ---------------------------
// What a v3 / v5 launch takes besides its instantiation.  Their 80 KB of
// dynamic LDS needs the attribute once per instantiation: each launcher sets
// it for the kernel it is about to launch, the first time it does.
struct GramCall {
  Gram3Plan p;
  const float* S;
  int N, K;
  float sc;
  float* part;
  hipStream_t st;
};

template <bool PRE, int NCP>
void launch_gram3(const GramCall& c, int lzs, const uint8_t* codes) {
  static const hipError_t attr =
      hipFuncSetAttribute(reinterpret_cast<const void*>(gram_kernel3<PRE, NCP>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, kG3Lds);
  (void)attr;
  hipLaunchKernelGGL((gram_kernel3<PRE, NCP>), dim3(c.p.ksplit * c.p.ngroups),
                     dim3(kG3Waves * kWave), kG3Lds, c.st, c.S, c.N, c.K, c.p.ns, c.p.t0s,
                     c.p.ntiles, c.p.ngroups, c.p.ksplit, c.p.nchunks, c.sc, c.part, lzs, codes);
}

// v5 / v6: the instantiation of the smallest rung >= T5 tiles per wave
// (gram5_plan keeps T5 <= 16 at W = 4, <= 8 at W = 8)
template <bool X3, int W>
void launch_gram5(int T5, const GramCall& c) {
  auto go = [&](auto rung) {
    constexpr int T = decltype(rung)::value;
    static const hipError_t attr =
        hipFuncSetAttribute(reinterpret_cast<const void*>(gram_kernel5<T, X3, W>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, kG3Lds);
    (void)attr;
    hipLaunchKernelGGL((gram_kernel5<T, X3, W>), dim3(((c.p.ksplit + 7) / 8 * 8) * c.p.ngroups),
                       dim3(W * kWave), kG3Lds, c.st, c.S, c.N, c.K, c.p.ns, c.p.t0s, c.p.ntiles,
                       c.p.ngroups, c.p.ksplit, c.p.nchunks, c.sc, c.part);
  };
  using std::integral_constant;
  if constexpr (W == 8) {
    if (T5 <= 4) go(integral_constant<int, 4>());
    else if (T5 <= 6) go(integral_constant<int, 6>());
    else if (T5 <= 7) go(integral_constant<int, 7>());
    else go(integral_constant<int, 8>());
  } else {
    if (T5 <= 4) go(integral_constant<int, 4>());
    else if (T5 <= 8) go(integral_constant<int, 8>());
    else if (T5 <= 10) go(integral_constant<int, 10>());
    else if (T5 <= 12) go(integral_constant<int, 12>());
    else if (T5 <= 13) go(integral_constant<int, 13>());
    else go(integral_constant<int, 16>());
  }
}
}  // namespace

// split-K partial buffer: the larger of the symmetric and full tile plans
int64_t part_bytes(int N, int64_t K) {
  int64_t b = 0;
  for (bool sym : {true, false}) {
    const GramPlan g = gram_plan(N, K, sym);
    b = std::max<int64_t>(b, (int64_t)((g.ksplit + 7) / 8 * 8) * g.npairs * 4096 * 4);
  }
  if (gram3_ok(N, K)) {
    // every skip (t0s) the v3 path can be given: more skipped tiles can
    // mean fewer groups and so more splits
    const int ns = (N + 31) / 32;
    for (int t0s = 0; t0s <= ns; ++t0s) {
      int T5;
      for (const Gram3Plan& g : {gram3_plan(N, K, t0s), gram5_plan(N, K, t0s, &T5),
                                 gram5_plan(N, K, t0s, &T5, 8)})
        b = std::max<int64_t>(b, (int64_t)g.ksplit * g.ntiles * 4096);
    }
  }
  return b;
}

int gram(const float* X, const float* Y, int N, int64_t K, int symmetric, float* G, float* part,
         hipStream_t st, int t0, float x3_max, bool pre, int lzs, const uint8_t* codes) {
  const GramPlan g = gram_plan(N, K, symmetric != 0, t0);
  if (g.npairs == 0) return TREX_OK;
  const bool x3 = x3_max > 0.0f;
  // the LDS-staged kernels (v3, v5) compute S S^T by 32-row strips
  const bool strips = symmetric && X == Y && gram3_ok(N, K);
  if (pre && !(x3 && strips))
    return set_error(TREX_E_UNSUPPORTED, "gram: no pre-split kernel for this shape");
  // v5 serves both precisions, v3 only the x3 one; pre-split operands: v3
  const int gv = pre ? 3 : gram_version(x3);
  if (strips && (x3 || gv >= 5)) {
    int T5 = 0;
    const int W = (gv == 6 && x3) ? 8 : kG5Waves;
    const Gram3Plan p = gv >= 5 ? gram5_plan(N, K, 2 * t0, &T5, W) : gram3_plan(N, K, 2 * t0);
    if (p.ntiles == 0) return TREX_OK;
    const GramCall c = {p, X, N, (int)K, x3 ? split_scale(x3_max) : 1.0f, part, st};
    if (gv >= 5 && !x3) {
      launch_gram5<false, kG5Waves>(T5, c);  // f32 -> v5: 587 -> 397 us at C5
    } else if (gv >= 5 && W == 8) {
      launch_gram5<true, 8>(T5, c);  // v6 (TREX_GRAM=6): measured, not adopted
    } else if (gv >= 5) {
      launch_gram5<true, kG5Waves>(T5, c);  // TREX_GRAM=5 only: x3 -> v3, v5 measured 231 vs 152 us
    } else {
      // code rows by compile-time passes of 128 rows (C5: 256 leaves, 2)
      const int ncp = (pre && codes && lzs > 0 && (32 * lzs) % kG3Rows4 == 0) ? 32 * lzs / kG3Rows4 : 0;
      if (!pre) launch_gram3<false, 0>(c, lzs, codes);
      else if (ncp == 1) launch_gram3<true, 1>(c, lzs, codes);
      else if (ncp == 2) launch_gram3<true, 2>(c, lzs, codes);
      else launch_gram3<true, 0>(c, lzs, codes);
    }
    hipLaunchKernelGGL(gram3_reduce_kernel, dim3(p.ntiles * 16), dim3(256), 0, st, part, N, p.ns,
                       p.t0s, p.ntiles, p.ksplit, G);
    return hip_check("gram");
  }
  // any other shape: one wave per 64x64 tile pair, v2 (K % 16 == 0) or v1
  const int blocks = g.npairs * ((g.ksplit + 7) / 8 * 8);
  if (K % 16 == 0 && x3) {
    const float sc = split_scale(x3_max);
    hipLaunchKernelGGL(gram_kernel2<true>, dim3(blocks), dim3(kWave), 0, st, X, Y, N, (int)K,
                       g.ntile, g.npairs, symmetric, t0, g.ksplit, g.kslice, part, sc, sc);
  } else if (K % 16 == 0)
    hipLaunchKernelGGL(gram_kernel2<false>, dim3(blocks), dim3(kWave), 0, st, X, Y, N, (int)K, g.ntile,
                       g.npairs, symmetric, t0, g.ksplit, g.kslice, part);
  else
    hipLaunchKernelGGL(gram_kernel, dim3(blocks), dim3(kWave), 0, st, X, Y, N, (int)K, g.ntile,
                       g.npairs, symmetric, t0, g.ksplit, g.kslice, part);
  hipLaunchKernelGGL(gram_reduce_kernel, dim3(grid_for((int64_t)g.npairs * 4096)), dim3(256), 0, st,
                     part, N, g.ntile, g.npairs, g.ksplit, symmetric, t0, G);
  return hip_check("gram");
}
}  // namespace trex

using namespace trex;

extern "C" int64_t trex_tree_workspace_bytes(int N, int64_t K) {
  if (N <= 0 || K <= 0) return 0;
  const int64_t part = part_bytes(N, K);
  const int64_t mats = (int64_t)N * N * 4 * 2;   // G, M
  const int64_t rows = (int64_t)N * 8 * 2 + 8192 * 8;  // row losses / E / norm parts
  return part + mats + rows + 1024;
}

// ---- split surrogate phases (for site-sharded multi-GPU: all-reduce G between
// trex_tree_gram and trex_tree_surrogate_combine) ----
extern "C" int trex_tree_gram_skip(const float* S, int N, int64_t K, int skip_rows, float* G,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
  if (!S || !G || !workspace || N <= 0 || K <= 0 || K > 0x7FFFFFFF || skip_rows < 0 ||
      skip_rows > N)
    return set_error(TREX_E_ARG, "trex_tree_gram_skip: bad arguments");
  if (workspace_bytes < trex_tree_workspace_bytes(N, K))
    return set_error(TREX_E_ARG, "trex_tree_gram_skip: workspace too small");
  return gram(S, S, N, K, 1, G, static_cast<float*>(workspace), (hipStream_t)stream,
              skip_rows / 64);
}

extern "C" int trex_tree_gram_skip_x3(const float* S, int N, int64_t K, int skip_rows,
                                      float max_abs, float* G, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
  if (!S || !G || !workspace || N <= 0 || K <= 0 || K > 0x7FFFFFFF || skip_rows < 0 ||
      skip_rows > N || !pos_finite_f32(max_abs))
    return set_error(TREX_E_ARG, "trex_tree_gram_skip_x3: bad arguments");
  if (K % 4 != 0)
    return set_error(TREX_E_UNSUPPORTED, "trex_tree_gram_skip_x3: K = L*Q must be a multiple of 4");
  if (workspace_bytes < trex_tree_workspace_bytes(N, K))
    return set_error(TREX_E_ARG, "trex_tree_gram_skip_x3: workspace too small");
  return gram(S, S, N, K, 1, G, static_cast<float*>(workspace), (hipStream_t)stream,
              skip_rows / 64, max_abs);
}

extern "C" int trex_tree_gram_mirror(float* G, int N, int row0, void* stream) {
  if (!G || N <= 0 || row0 < 0 || row0 > N)
    return set_error(TREX_E_ARG, "trex_tree_gram_mirror: bad arguments");
  if (row0 == 0 || row0 == N) return TREX_OK;
  const int64_t n = (int64_t)row0 * (N - row0);
  hipLaunchKernelGGL(gram_mirror_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1024)),
                     dim3(256), 0, (hipStream_t)stream, G, N, row0);
  return hip_check("trex_tree_gram_mirror");
}

extern "C" int trex_tree_gram(const float* S, int N, int64_t K, float* G, void* workspace,
                              int64_t workspace_bytes, void* stream) {
  return trex_tree_gram_skip(S, N, K, 0, G, workspace, workspace_bytes, stream);
}

extern "C" int trex_tree_split_x3(const float* X, int rows, int cols, int ldx, float max_abs,
                                  void* out, int ldo, void* stream) {
  if (!X || !out || rows <= 0 || cols <= 0 || ldx < cols || ldo < cols || ldo % 4 != 0 ||
      !pos_finite_f32(max_abs) || (reinterpret_cast<uintptr_t>(out) & 15) != 0)
    return set_error(TREX_E_ARG, "trex_tree_split_x3: bad arguments");
  const int64_t n = (int64_t)rows * (ldo / 4);
  hipLaunchKernelGGL(split_x3_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 65536)),
                     dim3(256), 0, (hipStream_t)stream, X, rows, cols, ldx, split_scale(max_abs),
                     static_cast<u32x4*>(out), ldo);
  return hip_check("trex_tree_split_x3");
}

extern "C" int trex_tree_gram_skip_x3p(const void* S16, int N, int64_t K, int skip_rows,
                                       float max_abs, float* G, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  if (!S16 || !G || !workspace || N <= 0 || K <= 0 || K > 0x7FFFFFFF || skip_rows < 0 ||
      skip_rows > N || !pos_finite_f32(max_abs) || K % 4 != 0)
    return set_error(TREX_E_ARG, "trex_tree_gram_skip_x3p: bad arguments");
  if (workspace_bytes < trex_tree_workspace_bytes(N, K))
    return set_error(TREX_E_ARG, "trex_tree_gram_skip_x3p: workspace too small");
  const float* S = static_cast<const float*>(S16);
  return gram(S, S, N, K, 1, G, static_cast<float*>(workspace), (hipStream_t)stream,
              skip_rows / 64, max_abs, true);
}

// the same Gram with the leaf rows declared exact one-hot by their codes
// (the buffer trex_tree_leaf_codes filled with status 0): their f16 lo plane
// is zero, so the lo x hi products of the leaf strips are skipped, and the
// code rows are read as their bytes instead of 16-B pre-split pieces
// (bitwise the plain call)
extern "C" int trex_tree_gram_skip_x3p_codes(const void* S16, int N, int64_t K, int skip_rows,
                                             float max_abs, const void* codes, int64_t codes_bytes,
                                             int n_leaf, int Q, float* G, void* workspace,
                                             int64_t workspace_bytes, void* stream) {
  if (!S16 || !G || !workspace || N <= 0 || K <= 0 || K > 0x7FFFFFFF || skip_rows < 0 ||
      skip_rows > N || !pos_finite_f32(max_abs) || K % 4 != 0)
    return set_error(TREX_E_ARG, "trex_tree_gram_skip_x3p_codes: bad arguments");
  const int lcr = trex_tree_leaf_code_rows(n_leaf);
  if (!codes || Q != 4 || lcr <= 0 || lcr > N || codes_bytes < (int64_t)lcr * (K / Q))
    return set_error(TREX_E_ARG, "trex_tree_gram_skip_x3p_codes: bad codes (Q = 4, n_leaf >= 32)");
  if (workspace_bytes < trex_tree_workspace_bytes(N, K))
    return set_error(TREX_E_ARG, "trex_tree_gram_skip_x3p_codes: workspace too small");
  const float* S = static_cast<const float*>(S16);
  // TREX_GRAM_LZ (A/B): 0 = every product computed, rows as pre-split f16;
  // 1 = zero-plane products skipped, rows pre-split; default: also the code
  // rows read as their bytes
  const int lz = env_int("TREX_GRAM_LZ", 2);
  const int lzs = lz == 0 ? 0 : lcr / 32;
  return gram(S, S, N, K, 1, G, static_cast<float*>(workspace), (hipStream_t)stream,
              skip_rows / 64, max_abs, true, lzs,
              lz >= 2 ? static_cast<const uint8_t*>(codes) : nullptr);
}
