// Fused forward + adjoint for Q = 4 softmin on a predecoded program
// (trex_fused4_program_build, plan.cpp; record layout: trex_common.h).
//
// The same work item, tables, slot stack, cache policies, ring depth and fp64
// partials as sankoff_kernel<4, true, 3> (sankoff_q4_dev.h), and the same
// arithmetic in the same order, so dp, tree_score and d_cost are bitwise the
// generic kernel's.  What differs is the step interpreter: the generic body
// decodes every step's descriptors on the scalar pipe, in both sweeps, for
// every one of a tree's tiles; here the planner has done that once and the
// loops switch on a step class and read operands (LDS byte offsets, re-read
// rows) from a 32-byte record.
//
// Workgroups are kF4Waves waves, one item each, on one copy of the leaf and
// pair tables, built once per workgroup: LDS is [tables][wave 0: slot stack,
// leaf tile][wave 1 ...] (sankoff_q4_dev.h), the records' offsets relative to a
// wave's corner.  Only the prologue has barriers; a wave without an item (a
// short last workgroup) passes them and leaves.
//
// Scope (route, sankoff.hip, checks it): uniform batch, tau > 0, leaf
// tile prefetchable (L % 4 == 0, <= 64 leaves), no site scores, marginals or
// ancestral states; a program exists (no sentinel child, unreached row or
// two-parent node).  The cost matrix decides on the device as in
// sankoff_kernel: the factored softmin runs the loops below, the per-row
// stabilised softmin (range(C) / tau > 40) the generic body.
#include <hip/hip_runtime.h>

#include "sankoff_dev.h"
#include "sankoff_q4_dev.h"
#include "trex_common.h"

namespace trex {

namespace {

struct F4Rec {
  int flags, row, a0, a1, slot, r0, r1;
};
__device__ __forceinline__ F4Rec load_rec(cptr<int> prog, int k) {
  const cptr<int> p = prog + kF4RecInts * k;
  return F4Rec{p[0], p[1], p[2], p[3], p[4], p[5], p[6]};
}

// wave: the wave's index in its workgroup; item: its item (-1: none)
template <bool SYM>
__device__ __forceinline__ void fused4_body(const KArgs& A, const int* prog_, float* lds, int wave,
                                            int item) {
  constexpr int Q = 4;
  constexpr int MODE = kSoftK;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int L = A.L;
  const float a = A.a, bcoef = A.bcoef;
  const int nb = A.nblocks;

  Coef<Q> cf;
  load_coef<Q, MODE>(A.cost, a, cf);

  // the workgroup's tables, then this wave's slot stack and leaf tile
  float* tab = lds;
  float* slots = f4_wave_lds(lds, wave, A.n_slots, A.nl);
  float* tm = tab + kLeafTabFloats;
  float* tu = tab + kLeafTabFloats + kPairFloats;
  float* tr = tab + kLeafTabFloats + 2 * kPairFloats;
  int8_t* lleaf = reinterpret_cast<int8_t*>(slots + (size_t)max(A.n_slots, 1) * Q * kWave);

  // ---- once per workgroup, one thread per entry (all of wave 0): leaf
  // tables, then pair tables (as sankoff_body) ----
  {
    float cmn, cmx;
    cost_range<Q>(A.cost, cmn, cmx);
    const float range = cmx - cmn;
    const bool lfast = (kSentinel - range) * a >= 64.0f;
    if (tid <= Q) {
      const cptr<float> cost = as_const(A.cost);
      float d1[Q], m1[Q], g1[Q], w1[Q][Q], gc1[Q];
#pragma unroll
      for (int j = 0; j < Q; ++j) {
        d1[j] = j == lane ? 0.0f : kSentinel;
        g1[j] = 1.0f;
      }
#pragma unroll
      for (int i = 0; i < Q; ++i)
#pragma unroll
        for (int j = 0; j < Q; ++j) w1[i][j] = 0.0f;
      if (lfast && lane < Q) {
#pragma unroll
        for (int i = 0; i < Q; ++i) {
          const float cv = cost[i * Q + lane];
          m1[i] = cv;
          const float ik = fast_exp2((cv - cf.cmin) * a);
#pragma unroll
          for (int j = 0; j < Q; ++j) w1[i][j] = j == lane ? ik : 0.0f;
        }
      } else {
        message<Q, MODE>(cf, a, bcoef, d1, m1);
        message_adjoint<Q, MODE>(cf, a, d1, g1, w1, gc1);
      }
#pragma unroll
      for (int i = 0; i < Q; ++i) {
        tab[lane * Q + i] = m1[i];
#pragma unroll
        for (int j = 0; j < Q; ++j) tab[kWTab + (lane * Q + i) * Q + j] = w1[i][j];
      }
    }
  }
  __syncthreads();  // T is written by threads <= Q
  if (tid < (Q + 1) * (Q + 1)) {
    const int c0 = lane / (Q + 1), c1 = lane - c0 * (Q + 1);
    float t0[Q], t1[Q], d1[Q], m1[Q], u[Q], rs[Q];
    lds_vec_get<Q>(tab + c0 * Q, t0);
    lds_vec_get<Q>(tab + c1 * Q, t1);
#pragma unroll
    for (int j = 0; j < Q; ++j) d1[j] = t0[j] + t1[j];
    message<Q, MODE, false>(cf, a, bcoef, d1, m1);
    lds_vec_put<Q>(tm + lane * Q, m1);
    softk_weights<Q, SYM>(cf, a, d1, u, rs);
    lds_vec_put<Q>(tu + lane * Q, u);
    lds_vec_put<Q>(tr + lane * Q, rs);
  }
  if (item < 0) {
    __syncthreads();  // the one below
    return;
  }

  // ---- this item ----
  const int tree = item / A.tiles;
  const int tile = item - tree * A.tiles;
  const int n_int = A.n_int;
  const size_t rows_base = (size_t)tree * n_int * L;
  const cptr<int> prog = as_const(prog_) + (size_t)tree * n_int * kF4RecInts;
  const int site = tile * kWave + lane;
  const bool active = site < L;

  // leaf tile: lane l loads dword (l & 15) of rows 4r + (l >> 4), 16 loads in
  // flight (the generic kernel's prefetch; L % 4 == 0 and nl <= 64 hold here)
  {
    const int pf_voff = (lane >> 4) * L + (lane & 15) * 4;
    const rsrc_t rl =
        make_rsrc(A.leaves + (size_t)tree * A.nl * L, (uint32_t)((size_t)A.nl * L));
    uint32_t pre[kPrefetchRows / 4];
#pragma unroll
    for (int r = 0; r < kPrefetchRows / 4; ++r)
      pre[r] = __builtin_amdgcn_raw_buffer_load_b32(rl, pf_voff, 4 * r * L + tile * kWave, kAuxLeaf);
    __syncthreads();  // the tables are written by a few threads, read by all
    uint32_t* dst = reinterpret_cast<uint32_t*>(lleaf);
#pragma unroll
    for (int r = 0; r < kPrefetchRows / 4; ++r) {
      const int row = 4 * r + (lane >> 4);
      if (row < A.nl) dst[row * 16 + (lane & 15)] = pre[r];
    }
  }

  const uint32_t treebytes = (uint32_t)((size_t)n_int * Q * L * 4);
  const rsrc_t rdp = make_rsrc(A.dp + rows_base * Q, treebytes);
  // inactive lanes address past the buffer: stores drop, loads return 0
  const int voff = active ? site * Q * 4 : 0x7FFFFFF0;
  const int rowbytes = L * Q * 4;

  // a lane's corner of the slot stack and of the leaf tile; the records hold
  // the byte offsets from there
  char* slot_l = reinterpret_cast<char*>(slots) + lane * (Q * 4);
  const int8_t* leaf_l = lleaf + lane;
  // a leaf's code, normalised to [0, Q] (Q: missing)
  auto rd_code = [&](int off) __attribute__((always_inline)) {
    const int code = ld_code(leaf_l + off);
    return ((unsigned)code < (unsigned)Q) ? code : Q;
  };
  auto rd_slot = [&](int off, float (&d)[Q]) __attribute__((always_inline)) {
    lds_vec_get<Q>(reinterpret_cast<const float*>(slot_l + off), d);
  };
  auto wr_slot = [&](int off, const float (&d)[Q]) __attribute__((always_inline)) {
    lds_vec_put<Q>(reinterpret_cast<float*>(slot_l + off), d);
  };

  // ---- forward ----
  float dv[Q];
  {
    float prev[Q];  // previous step's D / message (register bypass)
    F4Rec nxt = load_rec(prog, 0);
    for (int k = 0; k < n_int; ++k) {
      const F4Rec s = nxt;
      if (k + 1 < n_int) nxt = load_rec(prog, k + 1);
      const int fl = s.flags;
      const int fcls = (fl >> kF4FwdClassShift) & 15;
      int pair = 0;
      if (fcls <= kF4CherryDeferred) {
        // both codes in flight, then both table rows
        const int c0 = rd_code(s.a0), c1 = rd_code(s.a1);
        float t0[Q], t1[Q];
        lds_vec_get<Q>(tab + c0 * Q, t0);
        lds_vec_get<Q>(tab + c1 * Q, t1);
#pragma unroll
        for (int i = 0; i < Q; ++i) dv[i] = t0[i] + t1[i];
        pair = c0 * (Q + 1) + c1;
      } else if (fcls == kF4LeafInt) {
        const bool l0 = (fl & kF4Leaf0) != 0;
        const int code = rd_code(l0 ? s.a0 : s.a1);
        float d[Q], t[Q], m[Q];
        if (fl & (kF4Prev0 | kF4Prev1)) {
#pragma unroll
          for (int j = 0; j < Q; ++j) d[j] = prev[j];
        } else {
          rd_slot(l0 ? s.a1 : s.a0, d);
        }
        lds_vec_get<Q>(tab + code * Q, t);
        // a deferred cherry handed its message on (TM), not its D
        if (fl & (kF4Defer0 | kF4Defer1)) {
#pragma unroll
          for (int i = 0; i < Q; ++i) m[i] = d[i];
        } else {
          message<Q, MODE, false>(cf, a, bcoef, d, m);
        }
#pragma unroll
        for (int i = 0; i < Q; ++i) dv[i] = t[i] + m[i];
      } else {
        float d0[Q], d1[Q], m0[Q], m1[Q];
        if (fl & kF4Prev0) {
#pragma unroll
          for (int j = 0; j < Q; ++j) d0[j] = prev[j];
        } else {
          rd_slot(s.a0, d0);
        }
        if (fl & kF4Prev1) {
#pragma unroll
          for (int j = 0; j < Q; ++j) d1[j] = prev[j];
        } else {
          rd_slot(s.a1, d1);
        }
        if (fl & kF4Defer0) {
#pragma unroll
          for (int i = 0; i < Q; ++i) m0[i] = d0[i];
        } else {
          message<Q, MODE, false>(cf, a, bcoef, d0, m0);
        }
        if (fl & kF4Defer1) {
#pragma unroll
          for (int i = 0; i < Q; ++i) m1[i] = d1[i];
        } else {
          message<Q, MODE, false>(cf, a, bcoef, d1, m1);
        }
#pragma unroll
        for (int i = 0; i < Q; ++i) dv[i] = m0[i] + m1[i];
      }
      // deferred cherries' rows are never re-read: they stream (nt)
      if (fl & kF4DeferIn) {
        bst_row<Q, kAuxCherryRow>(rdp, voff, s.row * rowbytes, dv);
        // the row is stored; its one parent takes the message from the table
        lds_vec_get<Q>(tm + pair * Q, dv);
      } else {
        bst_row<Q, kAuxFusedRow>(rdp, voff, s.row * rowbytes, dv);
      }
      if (fl & kF4Put) wr_slot(s.slot, dv);
#pragma unroll
      for (int i = 0; i < Q; ++i) prev[i] = dv[i];
    }
  }

  // ---- root: score + cotangent ----
  float score, groot[Q];
  root_score<Q, true>(dv, a, bcoef, A.hard_root != 0, score, groot);
  {
    double tot = 0.0;
    if (active) tot += (double)score;
    tot = wave_sum_lane0(tot);
    if (lane == 0) A.part_tree[item] = tot;
  }

  // ---- adjoint ----
  // acc: dC accumulators of the factored form (x K[i][j] at the end)
  float acc[Q][Q];
  const float dscale = A.dts ? as_const(A.dts)[tree] : 1.0f;
  const float f = active ? dscale : 0.0f;
  float gnext[Q];  // cotangent handed to the next reverse step; the root's first
#pragma unroll
  for (int i = 0; i < Q; ++i) gnext[i] = groot[i] * f;
#pragma unroll
  for (int i = 0; i < Q; ++i)
#pragma unroll
    for (int j = 0; j < Q; ++j) acc[i][j] = 0.0f;

  // the DP rows a step re-reads are issued kAdjRing - 1 steps ahead, both
  // loads unconditionally (a row the step does not read is addressed past the
  // buffer: no traffic, zeros) so every path issues the same number of VMEM ops.
  // The program words of the reverse sweep (a step's re-read rows, its flags
  // and operand offsets) are read on the scalar pipe with no branch around the
  // load (a step before record 0 reads record 0 and ignores it) one step before
  // their first use, into rings with static indices
  struct F4Rows {
    int r0, r1;
  };
  struct F4Rev {
    int flags, a0, a1, slot;
  };
  auto load_rows = [&](int k) __attribute__((always_inline)) {
    const cptr<int> p = prog + kF4RecInts * max(k, 0);
    return F4Rows{p[5], p[6]};
  };
  auto load_rev = [&](int k) __attribute__((always_inline)) {
    const cptr<int> p = prog + kF4RecInts * max(k, 0);
    return F4Rev{p[0], p[2], p[3], p[4]};
  };
  // live: the rows are those of a step (k >= 0)
  auto pf_rows = [&](bool live, const F4Rows& w, float (&nd)[2][Q]) __attribute__((always_inline)) {
    const int r0 = live ? w.r0 : kF4NoRow, r1 = live ? w.r1 : kF4NoRow;
    bld_row<Q, kAuxFusedLoad>(rdp, r0 >= 0 ? voff : 0x7FFFFFF0, max(r0, 0) * rowbytes, nd[0]);
    bld_row<Q, kAuxFusedLoad>(rdp, r1 >= 0 ? voff : 0x7FFFFFF0, max(r1, 0) * rowbytes, nd[1]);
  };
  // acc_ij += g_i W[code][i][j] of a leaf child
  auto leaf_acc = [&](const float (&g)[Q], const float (&w)[Q * Q]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      float wr[Q];
#pragma unroll
      for (int j = 0; j < Q; ++j) wr[j] = w[i * Q + j];
      // (g_i through an opaque copy: otherwise the compiler builds the four
      // (g_i, g_i) pairs of the packed FMAs once per step, ahead of the class
      // branches, eight moves in every step, where a pair made inside the
      // leaf's block folds into the FMA's operand select; PERFLOG.md)
      float gi = g[i];
      asm volatile("" : "+v"(gi));
      axpy<Q>(acc[i], gi, wr);
    }
  };
  // edge to an internal child: its cotangent to the bypass or to its slot
  auto int_child = [&](bool deferred, bool prev, int off, const float (&d)[Q],
                       const float (&g)[Q]) __attribute__((always_inline)) {
    float gc[Q];
    if (deferred) {
      // the child's step runs this edge (kF4DeferIn)
#pragma unroll
      for (int j = 0; j < Q; ++j) gc[j] = g[j];
    } else {
      message_adjoint<Q, MODE, SYM>(cf, a, d, g, acc, gc);
    }
    if (prev) {
#pragma unroll
      for (int j = 0; j < Q; ++j) gnext[j] = gc[j];
    } else {
      wr_slot(off, gc);
    }
  };
  // ahead(): the scalar loads of the steps to come.  Called behind the step's
  // first LDS reads; the compiler sinks the loads to the join between the two
  // children's edges wherever they are written (PERFLOG.md), which still leaves
  // child 1's edge and the next step's prefetch arithmetic ahead of their use
  auto bstep = [&](const F4Rev& s, float (&cd)[2][Q], auto&& ahead) __attribute__((always_inline)) {
    const int fl = s.flags;
    float g[Q];
    if (fl & (kF4ToNext | kF4Root)) {
#pragma unroll
      for (int i = 0; i < Q; ++i) g[i] = gnext[i];
    } else {
      rd_slot(s.slot, g);
    }
    if (fl & kF4DeferIn) {
      // g is the parent's cotangent: the parent -> cherry edge first.  Its u
      // and 1 / s depend on the two leaf codes only (pair tables); both code
      // reads go out together
      const int c0 = rd_code(s.a0), c1 = rd_code(s.a1);
      const int pair = c0 * (Q + 1) + c1;
      float u[Q], rs[Q], gc[Q];
      lds_vec_get<Q>(tu + pair * Q, u);
      lds_vec_get<Q>(tr + pair * Q, rs);
      softk_edge<Q>(cf, u, rs, g, acc, gc);
#pragma unroll
      for (int i = 0; i < Q; ++i) g[i] = gc[i];
    }
    ahead();
    // the children in stored order (the dC sums depend on it).  One loop for
    // every class: straight-line code per class (a leaf's weights read beside
    // the other child's edge, a cherry's two weight tables and its edge tables
    // in one batch) measured 95 VGPRs or spills against 88 here, and the same
    // time (PERFLOG.md)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int off = c == 0 ? s.a0 : s.a1;
      if (fl & (c == 0 ? kF4Leaf0 : kF4Leaf1)) {
        const int code = rd_code(off);
        float w[Q * Q];
        lds_vec_get<Q * Q>(tab + kWTab + code * Q * Q, w);
        leaf_acc(g, w);
      } else {
        int_child((fl & (c == 0 ? kF4Defer0 : kF4Defer1)) != 0,
                  (fl & (c == 0 ? kF4Prev0 : kF4Prev1)) != 0, off, cd[c], g);
      }
    }
  };
  {
    // ring of kRing row buffers, unrolled so every buffer index is static.
    // Position r runs step k - r on buf[r] and rv[r]; it issues the rows of
    // step k - r - (kRing - 1) from rw[r] into the freed buffer, and loads the
    // next step's record and the next prefetch's rows into the next position
    constexpr int kRing = kAdjRing;
    float buf[kRing][2][Q];
    F4Rows rw[kRing];
    F4Rev rv[kRing];
#pragma unroll
    for (int r = 0; r < kRing - 1; ++r)
      pf_rows(n_int - 1 - r >= 0, load_rows(n_int - 1 - r), buf[r]);
    rw[0] = load_rows(n_int - kRing);
    rv[0] = load_rev(n_int - 1);
    for (int k = n_int - 1; k >= 0; k -= kRing) {
#pragma unroll
      for (int r = 0; r < kRing; ++r) {
        pf_rows(k - r - (kRing - 1) >= 0, rw[r], buf[(r + kRing - 1) % kRing]);
        if (k - r < 0) break;
        bstep(rv[r], buf[r], [&]() __attribute__((always_inline)) {
          rw[(r + 1) % kRing] = load_rows(k - r - kRing);
          rv[(r + 1) % kRing] = load_rev(k - r - 1);
        });
      }
    }
  }

  // ---- per-item dC partial (the fixed-order reduce kernel sums the items) ----
  double v16[16];
#pragma unroll
  for (int i = 0; i < Q; ++i)
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      v16[i * Q + j] = (double)acc[i][j];
      v16[i * Q + j] *= (double)cf.k[i][j];
    }
  const double v = wave_reduce_scatter16(v16, lane);
  if ((lane & 3) == 0) A.part_dc[(size_t)(lane >> 2) * nb + item] = v;
}

// Workgroups of XCD x (blockIdx % 8) take a contiguous range of the
// ceil(items / kF4Waves) item groups, wave w of a workgroup item
// kF4Waves * group + w: the waves of a workgroup, and of an XCD, work on
// adjacent tiles.  The items themselves (part_tree / part_dc) are numbered as
// in every Q <= 4 kernel.
__host__ __device__ inline int f4_groups(int items) { return (items + kF4Waves - 1) / kF4Waves; }

__global__ __launch_bounds__(kF4Waves * kWave)
__attribute__((amdgpu_waves_per_eu(kFusedWpe, kFusedWpeMax)))
void sankoff_fused4_kernel(KArgs A, const int* prog) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int groups = f4_groups(A.nblocks);
  const int per = (groups + 7) / 8;
  const int xcd = blockIdx.x & 7;
  const int group = xcd * per + (blockIdx.x >> 3);
  if (group >= min(groups, (xcd + 1) * per)) return;  // the whole workgroup
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  int item = group * kF4Waves + wave;
  if (item >= A.nblocks) item = -1;  // still passes every barrier
  float cmin, cmax;
  cost_range<4>(A.cost, cmin, cmax);
  if (use_ktrick(cmin, cmax, A.a)) {
    if (cost_symmetric<4>(A.cost))
      fused4_body<true>(A, prog, lds, wave, item);
    else
      fused4_body<false>(A, prog, lds, wave, item);
  } else {
    // the generic body per wave, on the same map: every wave writes the shared
    // tables (the same values) and keeps its own slot stack and leaf tile
    sankoff_body<4, kSoftDirect, 3, false, false, true>(
        A, lds, item, f4_wave_lds(lds, wave, A.n_slots, A.nl));
  }
}

}  // namespace

int g_fused4_launches = 0;  // tests: which kernel took a call

int fused4_run(const char* fn, const SankoffCall& c, const int32_t* prog, size_t lds) {
  const KArgs A = q4_args(c);
  const int grid = (f4_groups(A.nblocks) + 7) / 8 * 8;
  hipLaunchKernelGGL(sankoff_fused4_kernel, dim3(grid), dim3(kF4Waves * kWave), lds,
                     (hipStream_t)c.stream, A,
                     reinterpret_cast<const int*>(prog + TREX_PLAN_HEADER_INTS));
  ++g_fused4_launches;
  return hip_check(fn);
}

}  // namespace trex

extern "C" int trex_debug_fused4_launches(void) { return trex::g_fused4_launches; }
