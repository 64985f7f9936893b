// libtrexhip.so -- the tree-cost product dF = M F (tree.hip has the map of
// the tree-cost files).  Kernels: v2 (one wave per 64x64 tile, f32: any K),
// v3 (LDS-staged f16x3, persistent, two waves per SIMD: the x3 default, the
// only one for pre-split operands), v5 (one wave per SIMD: the f32 default),
// and the leaf codes the x3 kernels read in place of one-hot rows.  mf_x3()
// holds the one launch table.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "tree_dev.h"

namespace trex {
namespace {

// ---------------------------------------------------------------------------
// a9 dF = M F  (M [N][N], F [N][K]) on MFMA.  Column blocks are XCD-grouped:
// the row tiles of a column block share an XCD, so each F block leaves HBM
// once.
// ---------------------------------------------------------------------------

// v2 dF = M F (the f32-MFMA path; X3 = the first f16x3 version, kept
// instantiable for A/B builds, unused since MF v3): 16 n
// per step, next step's operands requested before this
// step's 32 MFMAs (ping-pong registers, unrolled by two).  Lane (r, h)
// supplies M[row][nb + 8h + t] and F[nb + 8h + t][col]; rows / n / cols past
// the edges read a clamped address and contribute 0 (M entry zeroed).
template <bool X3>
__global__ __launch_bounds__(kWave) void mf_kernel2(const float* __restrict__ Mm,
                                                   const float* __restrict__ F, int N, int K,
                                                   int row0, int nrows, int nrowt, int ncolb,
                                                   float* __restrict__ out, float sm = 1.0f,
                                                   float sf = 1.0f) {
  const int b = blockIdx.x;
  const int xcd = b & 7, m = b >> 3;
  const int rt = m % nrowt;
  const int cb = (m / nrowt) * 8 + xcd;
  if (cb >= ncolb) return;
  const int lane = threadIdx.x;
  const int r = lane & 31, h = lane >> 5;
  const int c0 = cb * 64;
  f32x16 acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) acc[u][v] = (f32x16){};
  // buffer (SRD) loads: lane part of the offset in voffset, the uniform n
  // part in soffset; rows of F past N and rows of M past N read out of
  // bounds (0); n past N within an M row is masked
  const rsrc_t rm = make_rsrc(Mm, (uint32_t)((size_t)N * N * 4));
  const rsrc_t rf = make_rsrc(F, (uint32_t)((size_t)N * K * 4));
  int mvo[2], fvo[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int row = rt * 64 + u * 32 + r;  // output row; M row row0 + row
    mvo[u] = row < nrows ? ((row0 + row) * N + 8 * h) * 4 : 0x7FFFFFF0;
    const int col = c0 + u * 32 + r;
    fvo[u] = ((8 * h) * K + (col < K ? col : K - 1)) * 4;
  }
  auto fetch = [&](int nb, float (&ma)[2][8], float (&fb)[2][8]) {
    // M[row][nb + 8h .. +8): two dwordx4 loads per row (rows are only 4-byte
    // aligned; buffer loads allow that); n past N masked to 0
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int hv = 0; hv < 2; ++hv) {
        const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(rm, mvo[u], (nb + 4 * hv) * 4, 0);
        const uint32_t e[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int t = 4 * hv + q;
          ma[u][t] = nb + 8 * h + t < N ? __uint_as_float(e[q]) : 0.0f;
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
#pragma unroll
      for (int v = 0; v < 2; ++v)
        fb[v][t] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rf, fvo[v], (nb + t) * K * 4, 0));
    }
  };
  auto compute = [&](int nb, float (&ma)[2][8], float (&fb)[2][8]) {
    if (nb >= N) return;
    if constexpr (X3) {
      h8 mh[2], ml[2], fh[2], fl[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) split_h8(ma[u], sm, mh[u], ml[u]);
#pragma unroll
      for (int v = 0; v < 2; ++v) split_h8(fb[v], sf, fh[v], fl[v]);
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = mfma_x3(mh[u], ml[u], fh[v], fl[v], acc[u][v]);
    } else {
#pragma unroll
      for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int v = 0; v < 2; ++v)
            acc[u][v] = __builtin_amdgcn_mfma_f32_32x32x2f32(ma[u][t], fb[v][t], acc[u][v], 0, 0, 0);
    }
  };
  float ma0[2][8], fb0[2][8], ma1[2][8], fb1[2][8];
  fetch(0, ma0, fb0);
  for (int nb = 0; nb < N; nb += 32) {
    fetch(nb + 16, ma1, fb1);
    compute(nb, ma0, fb0);
    fetch(nb + 32, ma0, fb0);
    compute(nb + 16, ma1, fb1);
  }
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = rt * 64 + u * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
        const int col = c0 + v * 32 + r;
        if (row < nrows && col < K) out[(size_t)row * K + col] = X3 ? acc[u][v][q] * (1.0f / (sm * sf)) : acc[u][v][q];
      }
}

// M row-major LDS image stride (bytes): hi n0..31 | lo n0..31 | pad
constexpr int kMfStride = 144;

typedef __fp16 fp16x4_t __attribute__((__vector_size__(4 * sizeof(__fp16))));
// two ds_read_b64_tr_b16 (rows k .. k+3 and k+4 .. k+7 of one 16-lane
// group's block) -> the 8-half B fragment of a 32x32x16 f16 MFMA
__device__ __forceinline__ h8 tr_pair(const unsigned char* p, int four_rows) {
  typedef __attribute__((address_space(3))) fp16x4_t lds_h4;
  const fp16x4_t a = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h4*)(p));
  const fp16x4_t b = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h4*)(p + four_rows));
  const h4 x = __builtin_bit_cast(h4, a), y = __builtin_bit_cast(h4, b);
  return (h8){x[0], x[1], x[2], x[3], y[0], y[1], y[2], y[3]};
}

// ---- v3 MF: out = M[row0 : row0 + nrows] F, LDS-staged, persistent --------
// A workgroup (8 waves, two per SIMD) owns TPC x 32 output columns per chunk
// and up to 256 output rows (wave w: rows 32w .. 32w + 31 x all TPC column
// tiles); persistent workgroups (one per CU) walk the column chunks
// blockIdx.x + i * gridDim.x with the load pipeline running straight across
// chunk boundaries, so one chunk's output stores overlap the next chunk's
// first loads.  n advances in stages of 32 (two 32x32x16 k-steps).  Per
// stage both operands are fetched ONCE per workgroup in full 128-B lines and
// split once into f16 hi / lo:
//   * F[n .. n+32)[chunk columns] (thread item (n, cg): F[n][4cg .. +3],
//     column groups fastest) -> ROW-major LDS planes [32 n][CW] (row stride
//     SF = CW * 2 rounded to 64 mod 256 bytes: conflict-free ds_write_b64
//     and transposed reads); a B fragment (8 n of one column) is two
//     ds_read_b64_tr_b16 per plane (gfx950's transposing LDS read: lane
//     4q+p of a 16-lane group addresses row q, columns 4p..4p+3; lane i
//     receives column i of the 4 rows);
//   * M[rows][n .. n+32) (thread t: row t / 8 + 64 i, n segment t % 8) ->
//     row-major LDS [256][144 B]; an A fragment is one ds_read_b128 per
//     plane.
// Two register sets (stages s+1, s+2 in flight), LDS double-buffered, one
// barrier per stage that waits on lgkmcnt only (__syncthreads() would drain
// the prefetch).  All offsets are in voffset: rows / n past N read out of
// bounds (0).  TPC (5 or 4) is picked per launch so column tiles divide
// evenly over the CUs (C5: 1 250 chunks of 5 tiles over 256 workgroups).
// Earlier versions (same box, tools/time_gemm.py): v2 (one wave per 64x64
// tile, operands from L2) 386 us; F staged column-major with 64-B row pieces
// per load + M fragments loaded per lane 320 us; + M staged in full lines
// 296 us; this 274 us.
// CODES (Q = 4): the n stages s < lcs (F rows 0 .. 32 lcs: exact one-hot leaf
// rows) load the rows' codes (codesR [32 lcs][L] bytes, trex_tree_leaf_codes;
// an F item = one site's 4 states = one byte) instead of F and expand them
// into the same f16 hi / lo planes (one-hot x sf is exact in f16, lo = 0):
// bitwise the same result, a quarter of the bytes for those stages
// PRE: M and F pre-split (split_x3_group layout; M rows ldm elements apart,
// zero past N): the stages copy them into LDS without the split arithmetic
template <int TPC, bool CODES, bool PRE = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void mf_kernel3(
    const float* __restrict__ Mm, const float* __restrict__ F, int N, int K, int row0, int nrows,
    int nchunks, float* __restrict__ out, float sm, float sf, const uint8_t* __restrict__ codesR,
    int lcs, int ldm) {
  constexpr int CW = TPC * 32;
  constexpr int NIT = 32 * (CW / 4);  // F (row, column group) float4 items per stage
  constexpr int IPT = (NIT + 511) / 512;
  constexpr int SF = (CW * 2 + 191) / 256 * 256 + 64;  // plane row stride (bytes)
  constexpr int FPLANE = 32 * SF;
  constexpr int FBUF = 2 * FPLANE;
  constexpr int MBUF = 256 * kMfStride;
  constexpr int BUF = FBUF + MBUF;
  extern __shared__ __attribute__((aligned(16))) unsigned char ldsm[];
  const int gx = gridDim.x;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 31, h = lane >> 5;
  const int rbase = blockIdx.y * 256 + wave * 32;
  const rsrc_t rm = make_rsrc(Mm, (uint32_t)((size_t)N * ldm * 4));
  const rsrc_t rf = make_rsrc(F, (uint32_t)((size_t)N * K * 4));
  // CODES: item (n, cg) reads the code byte of row n, site chunk * CW / 4 + cg
  // (sites past L read the next row's bytes: columns past K, never stored)
  const int Lc = K / 4;
  const rsrc_t rc = make_rsrc(codesR, (uint32_t)(CODES ? (size_t)Lc * 32 * lcs : 0));
  int cvb[IPT];
#pragma unroll
  for (int j = 0; j < IPT; ++j) {
    const int item = tid + 512 * j;
    cvb[j] = (item < NIT) ? (item / (CW / 4)) * Lc + item % (CW / 4) : 0x7FFF0000;
  }
  int fvb[IPT], lofs[IPT];
  bool fok[IPT];
#pragma unroll
  for (int j = 0; j < IPT; ++j) {
    const int item = tid + 512 * j;
    fok[j] = item < NIT;
    const int n = fok[j] ? item / (CW / 4) : 0, cg = fok[j] ? item % (CW / 4) : 0;
    fvb[j] = (n * K + 4 * cg) * 4;
    lofs[j] = n * SF + 8 * cg;
  }
  // M staging: thread t covers rows t / 8 + 64 i (i < 4), n segment t % 8
  const int mseg = tid & 7, mrow = tid >> 3;
  int mvb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rg = blockIdx.y * 256 + mrow + 64 * i;
    mvb[i] = rg < nrows ? ((row0 + rg) * ldm + 4 * mseg) * 4 : -1;
  }
  const int nst = (N + 31) / 32;
  const int cnt = blockIdx.x < nchunks ? (nchunks - 1 - (int)blockIdx.x) / gx + 1 : 0;
  const int G = cnt * nst;

  f32x16 acc[TPC];
#pragma unroll
  for (int t = 0; t < TPC; ++t) acc[t] = (f32x16){};

  struct Set { u32x4 a[IPT], m[4]; int s; };
  Set r0, r1;
  int fc = blockIdx.x, fs = 0;  // load cursor (chunk, stage)
  int cc = blockIdx.x, cs = 0;  // compute cursor
  auto load = [&](Set& q) {
    if (CODES && fs < lcs) {
      const int so = fs * 32 * Lc + fc * (CW / 4);
#pragma unroll
      for (int j = 0; j < IPT; ++j)
        q.a[j].x = __builtin_amdgcn_raw_buffer_load_b8(rc, cvb[j] < 0x7FFF0000 ? cvb[j] + so : cvb[j], 0, 0);
    } else {
      const int so = (fc * CW + fs * 32 * K) * 4;
#pragma unroll
      for (int j = 0; j < IPT; ++j) {
        const int vo = fok[j] ? fvb[j] + so : 0x7FFF0000;
        q.a[j] = __builtin_amdgcn_raw_buffer_load_b128(rf, vo, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      q.m[i] = __builtin_amdgcn_raw_buffer_load_b128(rm, mvb[i] < 0 ? 0x7FFF0000 : mvb[i] + fs * 128,
                                                     0, 0);
    q.s = fs;
    if (++fs == nst) { fs = 0; fc += gx; }
  };
  const uint32_t hb = (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)sf);  // one-hot 1 x sf
  auto stage = [&](unsigned char* buf, const Set& q) {
    if (CODES && q.s < lcs) {
#pragma unroll
      for (int j = 0; j < IPT; ++j) {
        if (!fok[j]) continue;
        const uint32_t code = q.a[j].x & 0xFFu;
        *reinterpret_cast<uint2*>(buf + lofs[j]) =
            uint2{(code == 0 ? hb : 0u) | ((code == 1 ? hb : 0u) << 16),
                  (code == 2 ? hb : 0u) | ((code == 3 ? hb : 0u) << 16)};
        // the lo plane (zero) is not staged: compute skips its products
      }
    }
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
      if (!fok[j] || (CODES && q.s < lcs)) continue;
      if constexpr (PRE) {
        *reinterpret_cast<uint2*>(buf + lofs[j]) = uint2{q.a[j].x, q.a[j].y};
        *reinterpret_cast<uint2*>(buf + FPLANE + lofs[j]) = uint2{q.a[j].z, q.a[j].w};
        continue;
      }
      const uint32_t e[4] = {q.a[j].x, q.a[j].y, q.a[j].z, q.a[j].w};
      h4 hi, lo;  // (the split stays spelled out: tree_dev.h)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float v = __uint_as_float(e[c]) * sf;
        hi[c] = (_Float16)v;
        lo[c] = (_Float16)(v - (float)hi[c]);
      }
      *reinterpret_cast<h4*>(buf + lofs[j]) = hi;
      *reinterpret_cast<h4*>(buf + FPLANE + lofs[j]) = lo;
    }
    unsigned char* mb = buf + FBUF;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (PRE) {
        unsigned char* rowp = mb + (mrow + 64 * i) * kMfStride + 8 * mseg;
        *reinterpret_cast<uint2*>(rowp) = uint2{q.m[i].x, q.m[i].y};
        *reinterpret_cast<uint2*>(rowp + 64) = uint2{q.m[i].z, q.m[i].w};
        continue;
      }
      const uint32_t e[4] = {q.m[i].x, q.m[i].y, q.m[i].z, q.m[i].w};
      h4 hi, lo;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float v = (q.s * 32 + 4 * mseg + c < N) ? __uint_as_float(e[c]) * sm : 0.0f;
        hi[c] = (_Float16)v;
        lo[c] = (_Float16)(v - (float)hi[c]);
      }
      unsigned char* row = mb + (mrow + 64 * i) * kMfStride + 8 * mseg;
      *reinterpret_cast<h4*>(row) = hi;
      *reinterpret_cast<h4*>(row + 64) = lo;
    }
  };
  // transposed-read lane address: group g = lane / 16, lane 4q + p of it
  // addresses row 8 (g / 2) + q, columns 16 (g % 2) + 4p .. + 3
  const int trk = 8 * (lane >> 5) + ((lane & 15) >> 2);
  const int trc = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  const float unscale = 1.0f / (sm * sf);
  auto compute = [&](const unsigned char* buf) {
    const unsigned char* pa = buf + FBUF + (wave * 32 + r) * kMfStride + 16 * h;
    // leaf-code stages: F's lo plane is zero (one-hot x sf is exact in f16),
    // so its ah x bl products -- exact zeros -- are skipped (bitwise).  The
    // build that staged the zero plane and computed every product was
    // removed at this commit; it can be rebuilt from its parent.
    const bool zlo = CODES && cs < lcs;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const h8 ah = *reinterpret_cast<const h8*>(pa + kk * 32);
      const h8 al = *reinterpret_cast<const h8*>(pa + kk * 32 + 64);
#pragma unroll
      for (int t = 0; t < TPC; ++t) {
        const int o1 = (kk * 16 + trk) * SF + (t * 32 + trc) * 2;
        const h8 bh = tr_pair(buf + o1, 4 * SF);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[t], 0, 0, 0);
        if (!zlo) {
          const h8 bl = tr_pair(buf + FPLANE + o1, 4 * SF);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[t], 0, 0, 0);
        }
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[t], 0, 0, 0);
      }
    }
    if (++cs == nst) {  // chunk done: store its tile, restart the accumulators
      if (rbase < nrows) {
#pragma unroll
        for (int t = 0; t < TPC; ++t) {
          const int col = cc * CW + t * 32 + r;
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int row = rbase + (q & 3) + 8 * (q >> 2) + 4 * h;
            if (row < nrows && col < K) out[(size_t)row * K + col] = acc[t][q] * unscale;
          }
        }
      }
#pragma unroll
      for (int t = 0; t < TPC; ++t) acc[t] = (f32x16){};
      cs = 0;
      cc += gx;
    }
  };

  if (G == 0) return;
  unsigned char* buf0 = ldsm;
  unsigned char* buf1 = ldsm + BUF;
  load(r0);
  load(r1);
  stage(buf0, r0);
  load(r0);
  lds_barrier();
  for (int g = 0; g < G; g += 2) {
    compute(buf0);
    if (g + 1 < G) stage(buf1, r1);
    load(r1);
    lds_barrier();
    if (g + 1 >= G) break;
    compute(buf1);
    if (g + 2 < G) stage(buf0, r0);
    load(r0);
    lds_barrier();
  }
}

// ---- v5 MF: one wave per SIMD, pipelined fragment reads --------------------
// v3's chunking, LDS images and leaf-code stages with Gram v5's structure: a
// workgroup is 4 waves (one per SIMD, accumulators in AGPRs), wave w owns
// output rows 64w .. 64w + 63 (two row tiles) x the chunk's TPC column tiles,
// so each B fragment (4 transposed reads) feeds 2 x 3 MFMAs and each A
// fragment TPC x 3.  One register set of raw operands: the stage-(s + 1)
// f16 split and the stage-(s + 2) loads ride between the stage-s MFMAs
// (one raw item after each column tile), with no branch in the stage body
// (loads past the split run on neighbouring data or out of bounds: 0, and
// stage into the buffer nobody reads next).
template <int TPC, bool CODES, bool X3>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void mf_kernel5(
    const float* __restrict__ Mm, const float* __restrict__ F, int N, int K, int row0, int nrows,
    int nchunks, float* __restrict__ out, float sm, float sf, const uint8_t* __restrict__ codesR,
    int lcs) {
  constexpr int CW = TPC * 32;
  constexpr int NIT = 32 * (CW / 4);  // F (row, column group) float4 items per stage
  constexpr int IPT = (NIT + 255) / 256;
  constexpr int SF = (CW * 2 + 191) / 256 * 256 + 64;  // plane row stride (bytes)
  constexpr int FPLANE = 32 * SF;
  // X3: f16 hi / lo planes [32 n][SF]; f32: the F slice transposed [CW][32 n]
  // (144-B columns: a lane's 8 n are two ds_read_b128, conflict-free)
  constexpr int FBUF = X3 ? 2 * FPLANE : CW * kMfStride;
  static_assert(X3 || !CODES, "leaf codes ride on the x3 path only");
  constexpr int MBUF = 256 * kMfStride;
  constexpr int BUF = FBUF + MBUF;
  constexpr int MPT = 8;  // M float4 items per thread: rows tid / 8 + 32 i
  constexpr int NRAW = IPT + MPT;
  extern __shared__ __attribute__((aligned(16))) unsigned char ldsm5[];
  const int gx = gridDim.x;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 31, h = lane >> 5;
  const int rbase = blockIdx.y * 256 + wave * 64;
  // M rows row0 .. row0 + nrows - 1 only: rows past them read out of bounds (0)
  const rsrc_t rm = make_rsrc(Mm + (size_t)row0 * N, (uint32_t)((size_t)nrows * N * 4));
  // output rows 0 .. nrows - 1: stores past them are dropped by the bounds check
  const rsrc_t ro = make_rsrc(out, (uint32_t)((size_t)nrows * K * 4));
  const rsrc_t rf = make_rsrc(F, (uint32_t)((size_t)N * K * 4));
  const int Lc = K / 4;
  const rsrc_t rc = make_rsrc(codesR, (uint32_t)(CODES ? (size_t)Lc * 32 * lcs : 0));
  static_assert(NIT % 256 == 0, "F items tile the workgroup exactly");
  int fvb[IPT], lofs[IPT], cvb[IPT];
#pragma unroll
  for (int j = 0; j < IPT; ++j) {
    const int item = tid + 256 * j;
    const int n = item / (CW / 4), cg = item % (CW / 4);
    fvb[j] = (n * K + 4 * cg) * 4;
    lofs[j] = X3 ? n * SF + 8 * cg : 4 * cg * kMfStride + 4 * n;
    cvb[j] = n * Lc + cg;
  }
  const int mseg = tid & 7, mrow = tid >> 3;
  const int mvb = ((blockIdx.y * 256 + mrow) * N + 4 * mseg) * 4;  // + i * 32 rows
  const int nst = (N + 31) / 32;
  const int cnt = blockIdx.x < nchunks ? (nchunks - 1 - (int)blockIdx.x) / gx + 1 : 0;
  const int G = cnt * nst;
  if (G == 0) return;

  f32x16 acc[2][TPC];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int t = 0; t < TPC; ++t) acc[u][t] = (f32x16){};

  u32x4 raw[NRAW];
  uint32_t rcode[CODES ? IPT : 1];
  // raw item i of (chunk fc, stage fs): F items first, then M.  CODES: a
  // leaf-code stage's F items come from the code bytes instead -- both loads
  // are issued, the unused one out of bounds (no memory request), so the
  // stage body has no branch
  auto load1 = [&](int i, int fc, int fs) {
    if (i < IPT) {
      const bool code = CODES && fs < lcs;
      const int so = __builtin_amdgcn_readfirstlane(code ? 0x7FFF0000 : (fc * CW + fs * 32 * K) * 4);
      raw[i] = __builtin_amdgcn_raw_buffer_load_b128(rf, fvb[i], so, 0);
      if (CODES) {
        const int sc = __builtin_amdgcn_readfirstlane(code ? fs * 32 * Lc + fc * (CW / 4) : 0x7FFF0000);
        rcode[i] = __builtin_amdgcn_raw_buffer_load_b8(rc, cvb[i], sc, 0);
      }
    } else {
      raw[i] = __builtin_amdgcn_raw_buffer_load_b128(
          rm, mvb, __builtin_amdgcn_readfirstlane(fs * 128 + (i - IPT) * 32 * N * 4), 0);
    }
  };
  // one-hot x sf is exact in f16 (sf a power of two <= 2^14): a code item's
  // hi plane is the one-hot pattern and its lo plane 0, as the f32 rows give
  auto stage1 = [&](unsigned char* buf, int i, int fs) {
    if (i < IPT) {
      float e[4] = {__uint_as_float(raw[i].x), __uint_as_float(raw[i].y),
                    __uint_as_float(raw[i].z), __uint_as_float(raw[i].w)};
      if (CODES) {
        const bool code = fs < lcs;
        const uint32_t cv = rcode[i] & 0xFFu;
#pragma unroll
        for (int c = 0; c < 4; ++c) e[c] = code ? (cv == (uint32_t)c ? 1.0f : 0.0f) : e[c];
      }
      if constexpr (!X3) {
#pragma unroll
        for (int c = 0; c < 4; ++c) *reinterpret_cast<float*>(buf + lofs[i] + c * kMfStride) = e[c];
        return;
      }
      h4 hi, lo;  // (the split stays spelled out: tree_dev.h)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float v = e[c] * sf;
        hi[c] = (_Float16)v;
        lo[c] = (_Float16)(v - (float)hi[c]);
      }
      *reinterpret_cast<h4*>(buf + lofs[i]) = hi;
      *reinterpret_cast<h4*>(buf + FPLANE + lofs[i]) = lo;
    } else {
      const int mi = i - IPT;
      const uint32_t e[4] = {raw[i].x, raw[i].y, raw[i].z, raw[i].w};
      if constexpr (!X3) {
        float4 v;
        v.x = (fs * 32 + 4 * mseg < N) ? __uint_as_float(e[0]) : 0.0f;
        v.y = (fs * 32 + 4 * mseg + 1 < N) ? __uint_as_float(e[1]) : 0.0f;
        v.z = (fs * 32 + 4 * mseg + 2 < N) ? __uint_as_float(e[2]) : 0.0f;
        v.w = (fs * 32 + 4 * mseg + 3 < N) ? __uint_as_float(e[3]) : 0.0f;
        *reinterpret_cast<float4*>(buf + FBUF + (mrow + 32 * mi) * kMfStride + 16 * mseg) = v;
        return;
      }
      h4 hi, lo;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float v = (fs * 32 + 4 * mseg + c < N) ? __uint_as_float(e[c]) * sm : 0.0f;
        hi[c] = (_Float16)v;
        lo[c] = (_Float16)(v - (float)hi[c]);
      }
      unsigned char* row = buf + FBUF + (mrow + 32 * mi) * kMfStride + 8 * mseg;
      *reinterpret_cast<h4*>(row) = hi;
      *reinterpret_cast<h4*>(row + 64) = lo;
    }
  };
  const int trk = 8 * (lane >> 5) + ((lane & 15) >> 2);
  const int trc = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  const float unscale = X3 ? 1.0f / (sm * sf) : 1.0f;

  // cursors: compute (cc, cs); staged stage = compute + 1; loaded = + 2
  int cc = blockIdx.x, cs = 0;
  int sc_ = cs + 1, scc = cc;  // staged-stage cursor
  if (sc_ == nst) { sc_ = 0; scc += gx; }
  int lc = scc, ls = sc_ + 1;  // load cursor
  if (ls == nst) { ls = 0; lc += gx; }
  unsigned char* buf0 = ldsm5;
  unsigned char* buf1 = ldsm5 + BUF;
#pragma unroll
  for (int i = 0; i < NRAW; ++i) load1(i, cc, cs);
#pragma unroll
  for (int i = 0; i < NRAW; ++i) {
    stage1(buf0, i, cs);
    load1(i, scc, sc_);
  }
  lds_barrier();
  for (int g = 0; g < G; ++g) {
    const unsigned char* cb = (g & 1) ? buf1 : buf0;
    unsigned char* nb = (g & 1) ? buf0 : buf1;
    const unsigned char* pa = cb + FBUF + (wave * 64 + r) * kMfStride + 16 * h;
    int item = 0;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      h8 ah[2], al[2];
      f32x8 fa[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if constexpr (X3) {
          ah[u] = *reinterpret_cast<const h8*>(pa + u * 32 * kMfStride + kk * 32);
          al[u] = *reinterpret_cast<const h8*>(pa + u * 32 * kMfStride + kk * 32 + 64);
        } else {  // n = 16 kk + 8 h .. + 7 (pa carries 16 h bytes: one more 16 h)
          fa[u] = *reinterpret_cast<const f32x8*>(pa + u * 32 * kMfStride + kk * 64 + 16 * h);
        }
      }
#pragma unroll
      for (int t = 0; t < TPC; ++t) {
        if constexpr (X3) {
          const int o1 = (kk * 16 + trk) * SF + (t * 32 + trc) * 2;
          const h8 bh = tr_pair(cb + o1, 4 * SF);
          const h8 bl = tr_pair(cb + FPLANE + o1, 4 * SF);
#pragma unroll
          for (int u = 0; u < 2; ++u) acc[u][t] = mfma_x3(ah[u], al[u], bh, bl, acc[u][t]);
        } else {
          // MFMA q covers n = 16 kk + q and 16 kk + 8 + q on the two lane halves
          const f32x8 fb = *reinterpret_cast<const f32x8*>(cb + (t * 32 + r) * kMfStride + kk * 64 + 32 * h);
#pragma unroll
          for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int q = 0; q < 8; ++q)
              acc[u][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[u][q], fb[q], acc[u][t], 0, 0, 0);
        }
        // one raw item per column tile: staged for stage + 1, refilled for + 2
        if (item < NRAW) {
          stage1(nb, item, sc_);
          load1(item, lc, ls);
          ++item;
        }
      }
    }
#pragma unroll
    for (int i = 2 * TPC; i < NRAW; ++i) {
      stage1(nb, i, sc_);
      load1(i, lc, ls);
    }
    if (++ls == nst) { ls = 0; lc += gx; }
    if (++sc_ == nst) { sc_ = 0; scc += gx; }
    if (++cs == nst) {  // chunk done: store its tiles, restart the accumulators
      // branch-free: columns past K (a ragged last tile) get an out-of-
      // bounds offset, rows past nrows fall outside the store resource
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int t = 0; t < TPC; ++t) {
          const int col = cc * CW + t * 32 + r;
          const int row = rbase + u * 32 + 4 * h;
          const int vo = (col < K && row < nrows) ? (row * K + col) * 4 : 0x7FFFFFF0;
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int dr = (q & 3) + 8 * (q >> 2);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[u][t][q] * unscale), ro,
                                                  vo, __builtin_amdgcn_readfirstlane(dr * K * 4), 0);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int t = 0; t < TPC; ++t) acc[u][t] = (f32x16){};
      cs = 0;
      cc += gx;
    }
    lds_barrier();
  }
}

int cu_count() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
      v = 256;
    return v;
  }();
  return n;
}

// TREX_MF: 3 sends f32 calls to the one-wave-per-tile kernel (v2), 5 sends x3
// calls to v5; anything else: f32 -> v5 (one wave per SIMD, 525 -> 467 us at
// C5), x3 -> v3 (v5 measured 242 vs 224 us with leaf codes at C5)
int mf_version(bool x3) {
  const int e = env_int("TREX_MF", 0);
  return x3 ? (e == 5 ? 5 : 3) : (e == 3 ? 3 : 5);
}

// ---- the launch table of the LDS-staged kernels ---------------------------
// What a v3 / v5 launch takes besides its instantiation (ct: column tiles of
// 32 in all, rg: row groups of 256 output rows).
struct MfCall {
  const float *M, *S;
  int N, K, row0, nrows;
  float* out;
  float sm, sf;
  const uint8_t* codesR;
  int lcs, ldm;
  int64_t ct;
  int rg;
  hipStream_t st;
};

// column tiles per workgroup: fewest rounds x tiles over one workgroup per CU
int mf_tpc(int64_t ct, int rg) {
  int best = 5;
  int64_t best_cost = INT64_MAX;
  for (int tpc : {5, 4}) {
    const int64_t wgs = (ct + tpc - 1) / tpc * rg;
    const int64_t cost = (wgs + cu_count() - 1) / cu_count() * tpc;
    if (cost < best_cost) { best_cost = cost; best = tpc; }
  }
  return best;
}

// One launch: a persistent workgroup per CU (per row group) over the chunks
// of TPC tiles.  VER 3: B = PRE; VER 5: B = X3 (the f32 v5 has no leaf
// codes).  More than 64 KB of dynamic LDS needs the attribute, set once per
// instantiation.
template <int VER, int TPC, bool CODES, bool B>
void launch_mf(const MfCall& c) {
  static_assert(VER == 3 || VER == 5, "MF kernel version");
  // two buffers of F hi / lo planes + M; f32 v5: the transposed F slice, CW x 144 B
  constexpr int lds = (VER == 5 && !B) ? 2 * (160 * kMfStride + 256 * kMfStride)
                                       : 2 * (2 * 32 * 320 + 256 * kMfStride);
  const int nch = (int)((c.ct + TPC - 1) / TPC);
  const dim3 grid(std::max(1, std::min(nch, std::max(1, cu_count() / c.rg))), c.rg);
  auto go = [&](auto kernel, int threads, auto... tail) {
    static const hipError_t attr = hipFuncSetAttribute(
        reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)attr;
    hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, c.st, c.M, c.S, c.N, c.K, c.row0,
                       c.nrows, nch, c.out, c.sm, c.sf, c.codesR, c.lcs, tail...);
  };
  if constexpr (VER == 3) go(mf_kernel3<TPC, CODES, B>, 512, c.ldm);
  else go(mf_kernel5<TPC, CODES, B>, 256);
}

// (version, TPC, CODES, PRE / X3) -> the instantiation
template <int TPC, bool CODES>
void dispatch_mf(int ver, bool x3, bool pre, const MfCall& c) {
  if (ver == 5 && x3) launch_mf<5, TPC, CODES, true>(c);
  else if (ver == 5) launch_mf<5, TPC, false, false>(c);
  else if (pre) launch_mf<3, TPC, CODES, true>(c);
  else launch_mf<3, TPC, CODES, false>(c);
}

// the x3 / pre-split / f32-v5 MF; codesR / lcs: leaf-code stages (CODES
// instantiation) or null / 0
int mf_x3(const char* fn, const float* M, const float* S, int N, int64_t K, int row0, int nrows,
          float max_abs_m, float max_abs_s, float* dS_rows, const uint8_t* codesR, int lcs,
          void* stream, bool x3, bool pre = false, int ldm = 0) {
  if (!pre) ldm = N;
  if (!M || !S || !dS_rows || N <= 0 || K <= 0 || K > 0x7FFFFFFF || row0 < 0 || nrows <= 0 ||
      row0 + nrows > N || !pos_finite_f32(max_abs_m) || !pos_finite_f32(max_abs_s))
    return set_error(TREX_E_ARG, "%s: bad arguments", fn);
  if ((int64_t)N * K * 4 > 0x7FFFFFF0LL)
    return set_error(TREX_E_UNSUPPORTED, "%s: S exceeds 2 GiB", fn);
  // float4 operand loads: rows must start 16-B aligned (the last column tile
  // may be ragged: its columns past K are computed from the next row's data
  // and never stored)
  if (K % 4 != 0)
    return set_error(TREX_E_UNSUPPORTED, "%s: K = L*Q must be a multiple of 4", fn);
  // v5's dropped stores carry an out-of-bounds voffset plus a row soffset
  // (< 32 K * 4 bytes): kept below 2^31 so the sum cannot wrap in bounds
  const bool v5_ok = 32LL * K * 4 < 0x7FFFFFF0LL;
  if (!x3 && !v5_ok) return set_error(TREX_E_UNSUPPORTED, "%s: K too large for the f32 v5 MF", fn);
  if (pre && (!x3 || ldm < N || ldm % 32 != 0 || (int64_t)N * ldm * 4 > 0x7FFFFFF0LL))
    return set_error(TREX_E_ARG, "%s: bad pre-split M stride", fn);
  // f32: v5 (the caller has taken TREX_MF=3 to v2); x3: v3 unless TREX_MF=5;
  // pre-split operands: the v3 kernel
  const int ver = (!pre && v5_ok && (!x3 || mf_version(true) == 5)) ? 5 : 3;
  const MfCall c = {M, S, N, (int)K, row0, nrows, dS_rows,
                    x3 ? split_scale(max_abs_m) : 1.0f, x3 ? split_scale(max_abs_s) : 1.0f,
                    codesR, lcs, ldm, (K + 31) / 32, (nrows + 255) / 256, (hipStream_t)stream};
  const bool codes = codesR && lcs > 0;
  if (mf_tpc(c.ct, c.rg) == 5) {
    if (codes) dispatch_mf<5, true>(ver, x3, pre, c);
    else dispatch_mf<5, false>(ver, x3, pre, c);
  } else {
    if (codes) dispatch_mf<4, true>(ver, x3, pre, c);
    else dispatch_mf<4, false>(ver, x3, pre, c);
  }
  return hip_check(fn);
}
}  // namespace

void launch_mf2(const float* M, const float* S, int N, int K, int row0, int nrows, float* out,
                hipStream_t st) {
  const int nrowt = (nrows + 63) / 64;
  const int ncolb = (K + 63) / 64;
  const int blocks = nrowt * ((ncolb + 7) / 8 * 8);
  hipLaunchKernelGGL(mf_kernel2<false>, dim3(blocks), dim3(kWave), 0, st, M, S, N, K, row0, nrows,
                     nrowt, ncolb, out);
}
}  // namespace trex

using namespace trex;

namespace {  // (not trex::: profiles quote the kernel by this name)
// leaf codes of rows [0, lcr): codesR [lcr][L] bytes, the state of each
// exactly one-hot (row, site); 0xFF and *status = 1 otherwise
__global__ __launch_bounds__(256) void leaf_codes_kernel(const float* __restrict__ S, int L, int lcr,
                                                         uint8_t* __restrict__ codesR,
                                                         int* __restrict__ status) {
  const int64_t n = (int64_t)lcr * L;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
    const float4 v = reinterpret_cast<const float4*>(S)[t];  // row t / L, site t % L, Q = 4
    const float e[4] = {v.x, v.y, v.z, v.w};
    int ones = 0, idx = 0;
    bool clean = true;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (e[q] == 1.0f) {
        ++ones;
        idx = q;
      } else if (e[q] != 0.0f) {
        clean = false;
      }
    }
    const bool ok = clean && ones == 1;
    codesR[t] = ok ? (uint8_t)idx : (uint8_t)0xFF;
    if (!ok) atomicOr(status, 1);
  }
}
}  // namespace

extern "C" int trex_tree_mf_rows(const float* M, const float* S, int N, int64_t K, int row0,
                                 int nrows, float* dS_rows, void* stream) {
  if (!M || !S || !dS_rows || N <= 0 || K <= 0 || K > 0x7FFFFFFF || row0 < 0 || nrows <= 0 ||
      row0 + nrows > N)
    return set_error(TREX_E_ARG, "trex_tree_mf_rows: bad arguments");
  if ((int64_t)N * K * 4 > 0x7FFFFFF0LL)
    return set_error(TREX_E_UNSUPPORTED, "trex_tree_mf_rows: S exceeds 2 GiB");
  // v5 f32 needs K % 4 == 0 (16-B rows); TREX_MF=3 or a ragged K: the
  // one-wave-per-tile kernel
  if (K % 4 == 0 && 32LL * K * 4 < 0x7FFFFFF0LL && mf_version(false) == 5)
    return mf_x3("trex_tree_mf_rows", M, S, N, K, row0, nrows, 1.0f, 1.0f, dS_rows, nullptr, 0,
                 stream, false);
  launch_mf2(M, S, N, (int)K, row0, nrows, dS_rows, (hipStream_t)stream);
  return hip_check("trex_tree_mf_rows");
}

extern "C" int trex_tree_mf_rows_x3(const float* M, const float* S, int N, int64_t K, int row0,
                                    int nrows, float max_abs_m, float max_abs_s, float* dS_rows,
                                    void* stream) {
  return mf_x3("trex_tree_mf_rows_x3", M, S, N, K, row0, nrows, max_abs_m, max_abs_s, dS_rows,
               nullptr, 0, stream, true);
}

extern "C" int trex_tree_leaf_code_rows(int n_leaf) { return n_leaf >= 32 ? 32 * (n_leaf / 32) : 0; }

extern "C" int64_t trex_tree_leaf_codes_bytes(int n_leaf, int L) {
  const int64_t lcr = trex_tree_leaf_code_rows(n_leaf);
  return (L <= 0 || lcr <= 0) ? 0 : lcr * L;
}

extern "C" int trex_tree_leaf_codes(const float* S, int n_leaf, int L, int Q, void* codes,
                                    int64_t codes_bytes, int* status, void* stream) {
  const int lcr = trex_tree_leaf_code_rows(n_leaf);
  if (!S || !codes || !status || L <= 0 || Q != 4 || lcr <= 0 ||
      (reinterpret_cast<uintptr_t>(S) & 15) != 0)
    return set_error(TREX_E_ARG, "trex_tree_leaf_codes: bad arguments (Q = 4, n_leaf >= 32, 16-B aligned S)");
  if (codes_bytes < trex_tree_leaf_codes_bytes(n_leaf, L))
    return set_error(TREX_E_ARG, "trex_tree_leaf_codes: codes buffer too small");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess)
    return set_error(TREX_E_HIP, "trex_tree_leaf_codes: memset failed");
  const int64_t n = (int64_t)lcr * L;
  hipLaunchKernelGGL(leaf_codes_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 8192)),
                     dim3(256), 0, st, S, L, lcr, static_cast<uint8_t*>(codes), status);
  return hip_check("trex_tree_leaf_codes");
}

extern "C" int trex_tree_mf_rows_x3_codes(const float* M, const float* S, int N, int64_t K,
                                          int row0, int nrows, float max_abs_m, float max_abs_s,
                                          const void* codes, int64_t codes_bytes, int n_leaf,
                                          int Q, float* dS_rows, void* stream) {
  const int lcr = trex_tree_leaf_code_rows(n_leaf);
  if (!codes || lcr <= 0 || lcr > N || Q != 4 || K % 4 != 0)
    return set_error(TREX_E_ARG, "trex_tree_mf_rows_x3_codes: bad arguments (Q = 4 codes only)");
  // one code byte per (code row, site): the buffer trex_tree_leaf_codes filled
  if (codes_bytes < (int64_t)lcr * (K / Q))
    return set_error(TREX_E_ARG, "trex_tree_mf_rows_x3_codes: codes buffer smaller than "
                                 "trex_tree_leaf_codes_bytes(n_leaf, K / Q)");
  return mf_x3("trex_tree_mf_rows_x3_codes", M, S, N, K, row0, nrows, max_abs_m, max_abs_s,
               dS_rows, static_cast<const uint8_t*>(codes), lcr / 32, stream, true);
}

extern "C" int trex_tree_mf_rows_x3p(const void* M16, int ldm, const void* S16, int N, int64_t K,
                                     int row0, int nrows, float max_abs_m, float max_abs_s,
                                     const void* codes, int64_t codes_bytes, int n_leaf, int Q,
                                     float* dS_rows, void* stream) {
  const char* fn = "trex_tree_mf_rows_x3p";
  if (K % 4 != 0 || (codes && Q != 4)) return set_error(TREX_E_ARG, "%s: bad arguments", fn);
  int lcs = 0;
  if (codes) {
    const int lcr = trex_tree_leaf_code_rows(n_leaf);
    if (lcr <= 0 || lcr > N || codes_bytes < (int64_t)lcr * (K / Q))
      return set_error(TREX_E_ARG, "%s: bad codes", fn);
    lcs = lcr / 32;
  }
  return mf_x3(fn, static_cast<const float*>(M16), static_cast<const float*>(S16), N, K, row0,
               nrows, max_abs_m, max_abs_s, dS_rows, static_cast<const uint8_t*>(codes), lcs,
               stream, true, true, ldm);
}

extern "C" int trex_tree_mf(const float* M, const float* S, int N, int64_t K, float* dS,
                            void* stream) {
  return trex_tree_mf_rows(M, S, N, K, 0, N, dS, stream);
}
