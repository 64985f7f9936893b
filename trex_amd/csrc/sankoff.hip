// libtrexhip.so -- Sankoff DP kernels for MI355X (gfx950, CDNA4).
//
// Reference semantics: maraxen/trex src/trex/sankoff.py (run_dp :24-94,
// vectorized_dp :97, run_sankoff :114-188, backtrack_sankoff_jit :191-267).
// Design: one 64-lane wave per workgroup owns 64 consecutive
// sites of ONE tree (one per lane), so every branch on the topology is
// wave-uniform and the per-tree program (plan.cpp) is read with scalar loads.
// Live internal DP
// vectors / cotangents sit in a per-lane LDS stack (Sethi-Ullman slots);
// the DP table is streamed to HBM with sites innermost (16/8-byte stores).
// The cost matrix (and exp(-(C-cmin)/tau)) live in SGPRs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <mutex>

#include "sankoff_dev.h"
#include "sankoff_q4_dev.h"
#include "trex_common.h"

namespace trex {

static thread_local char g_err[512] = "no error";

int set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int hip_check(const char* fn) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(TREX_E_HIP, "%s: %s", fn, hipGetErrorString(e));
  return TREX_OK;
}

void tau_coefs(float tau, float* a, float* bcoef) {
  if (tau > 0.0f) {
    *a = (float)(1.4426950408889634 / (double)tau);
    *bcoef = (float)((double)tau * 0.6931471805599453);
  } else {
    *a = 0.0f;
    *bcoef = 0.0f;
  }
}

namespace {

template <int Q, bool SOFT, int PHASE, bool RAGGED = false>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(
    PHASE == 1 ? kFwdWpe : PHASE == 2 ? kAdjWpe : kFusedWpe, PHASE == 3 ? kFusedWpeMax : 8)))
void sankoff_kernel(KArgs A) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if constexpr (!SOFT) {
    sankoff_body<Q, kHard, PHASE, RAGGED>(A, lds);
  } else {
    float cmin, cmax;
    cost_range<Q>(A.cost, cmin, cmax);
    if (use_ktrick(cmin, cmax, A.a)) {
      // the adjoint-bearing kernels (the forward-only one measured no gain
      // and would carry a third body's scalar registers: 154 -> 245 spilled)
      if ((PHASE & 2) && cost_symmetric<Q>(A.cost))
        sankoff_body<Q, kSoftK, PHASE, RAGGED, true>(A, lds);
      else
        sankoff_body<Q, kSoftK, PHASE, RAGGED>(A, lds);
    } else
      sankoff_body<Q, kSoftDirect, PHASE, RAGGED>(A, lds);
  }
}

// --------------------------------------------------------------------------
// trex-exact ancestral reconstruction (sankoff.py:166-185, 191-267) of a
// ragged Q <= 4 batch, one lane per site (uniform batches: wide_backtrack).
// rmeta points at the ragged plan's records; the item table follows them,
// then the steps and the backtrack entries (see plan.cpp)
// --------------------------------------------------------------------------
template <int Q>
__global__ __launch_bounds__(kWave) void sankoff_ragged_backtrack_kernel(
    const int* __restrict__ rmeta, const float* __restrict__ cost, const float* __restrict__ dp,
    int8_t* __restrict__ anc, int B, int items, int steps) {
  const int item = blockIdx.x;
  const int tree = as_const(rmeta + (size_t)B * kRaggedMeta)[item];
  const cptr<int> m = as_const(rmeta) + (size_t)tree * kRaggedMeta;
  const int n_int = m[1];
  const int L = m[3];
  const int tile = item - m[5];
  const size_t rows_base = (size_t)(uint32_t)m[8] | ((size_t)(uint32_t)m[9] << 32);
  const int2* bt =
      reinterpret_cast<const int2*>(rmeta + (size_t)B * kRaggedMeta + items + (size_t)steps * 4) +
      m[0];
  const int lane = threadIdx.x;
  const int site = tile * kWave + lane;
  if (site >= L) return;
  float c[Q][Q];
#pragma unroll
  for (int i = 0; i < Q; ++i)
#pragma unroll
    for (int j = 0; j < Q; ++j) c[i][j] = as_const(cost)[i * Q + j];
  const cptr<int> prog = as_const(reinterpret_cast<const int*>(bt));
  const size_t rowstride = (size_t)Q * L;  // site-major rows [L][Q]
  const float* dpt = dp + rows_base * Q + (size_t)site * Q;
  int8_t* at = anc + rows_base + site;
  for (int k = 0; k < n_int; ++k) {
    const int2 e = make_int2(prog[2 * k], prog[2 * k + 1]);
    const int x = e.x & 0xFFFF;
    const int kind = (e.x >> 16) & 0xF;
    int out = 0;
    if (kind != kBtUnreached) {
      float d[Q];
      if (kind == kBtSentinel) {
#pragma unroll
        for (int j = 0; j < Q; ++j) d[j] = kSentinel;
      } else {
        const float* pr = dpt + (size_t)x * rowstride;
        if constexpr (Q == 4) {
          const float4 v = *reinterpret_cast<const float4*>(pr);
          d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        } else {
#pragma unroll
          for (int j = 0; j < Q; ++j) d[j] = pr[j];
        }
      }
      if (kind == kBtRoot) {
        float bv = d[0];
#pragma unroll
        for (int j = 1; j < Q; ++j)
          if (d[j] < bv) { bv = d[j]; out = j; }
      } else {
        const int sp = ld_code(at + (size_t)e.y * L);  // the parent's state
        float row[Q];
#pragma unroll
        for (int j = 0; j < Q; ++j) {
          float v = c[0][j];
#pragma unroll
          for (int i = 1; i < Q; ++i) v = (sp == i) ? c[i][j] : v;
          row[j] = v;
        }
        float bv = row[0] + d[0];
#pragma unroll
        for (int j = 1; j < Q; ++j) {
          const float v = row[j] + d[j];
          if (v < bv) { bv = v; out = j; }
        }
      }
    }
    st_code(at + (size_t)x * L, out);
  }
}

// dp [B][n_int][L][Q] (site-major, every Q) -> trex VmappedDPTable [B][L][n_all][Q]
__global__ __launch_bounds__(256) void to_trex_layout_kernel(const float* __restrict__ dp,
                                                            const int8_t* __restrict__ leaves,
                                                            int B, int L, int n_all, int nl, int Q,
                                                            float* __restrict__ out) {
  const size_t total = (size_t)B * n_all * L;
  const int ni = n_all - nl;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (size_t)gridDim.x * blockDim.x) {
    const int l = (int)(t % L);
    const size_t rest = t / L;
    const int node = (int)(rest % n_all);
    const int b = (int)(rest / n_all);
    float* o = out + (((size_t)b * L + l) * n_all + node) * Q;
    if (node < nl) {
      const int code = leaves[((size_t)b * nl + node) * L + l];
      for (int q = 0; q < Q; ++q) o[q] = (code == q) ? 0.0f : kSentinel;
    } else {
      const float* src = dp + (((size_t)b * ni + (node - nl)) * L + l) * Q;
      for (int q = 0; q < Q; ++q) o[q] = src[q];
    }
  }
}

// --------------------------------------------------------------------------
// host launch helpers
// --------------------------------------------------------------------------
struct Shape {
  int B, L, n_all, nl, ni, Q;
};

int check_shape(const char* fn, int B, int L, int n_all, int Q, Shape* sh) {
  if (B <= 0 || L <= 0 || n_all < 3 || n_all > 65535 || Q < 2)
    return set_error(TREX_E_ARG, "%s: bad shape B=%d L=%d n_all=%d Q=%d", fn, B, L, n_all, Q);
  if (Q > kBigMaxQ)
    return set_error(TREX_E_UNSUPPORTED, "%s: Q=%d > %d not supported by this build (int8 leaf "
                     "codes / ancestral states)", fn, Q, kBigMaxQ);
  sh->B = B;
  sh->L = L;
  sh->n_all = n_all;
  sh->nl = tree_nl(n_all);
  sh->ni = tree_ni(n_all);
  sh->Q = Q;
  return TREX_OK;
}

size_t lds_bytes(int n_slots, int nl, int Q, int phase) {
  const size_t b = (size_t)tab_floats(phase) * 4 +
                   (size_t)std::max(n_slots, 1) * Q * kWave * 4 + (size_t)nl * kWave;
  return (b + 15) & ~(size_t)15;
}

int device_cus() {
  static const int cus = [] {
    int dev = 0, n = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    return n;
  }();
  return cus;
}

// persistent grid: as many single-wave blocks as are co-resident (occupancy
// x CUs), a multiple of 8 (one share per XCD), never more than the items
template <class K>
int persistent_grid(K kernel, size_t lds, int nitems) {
  static std::mutex mu;
  struct Entry { const void* k; size_t lds; int occ; };
  static Entry cache[64];
  static int ncache = 0;
  int occ = 0;
  {
    std::lock_guard<std::mutex> g(mu);
    for (int i = 0; i < ncache; ++i)
      if (cache[i].k == (const void*)kernel && cache[i].lds == lds) occ = cache[i].occ;
    if (occ == 0) {
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, kWave, lds) != hipSuccess ||
          occ <= 0)
        occ = 4;
      if (ncache < 64) cache[ncache++] = Entry{(const void*)kernel, lds, occ};
    }
  }
  const long resident = (long)device_cus() * occ / 8 * 8;
  const long want = ((long)nitems + 7) / 8 * 8;
  return (int)std::max(8L, std::min(resident, want));
}

// one site per lane: two doubled the adjoint's VGPRs and were slower at every
// grid measured
template <int Q, bool SOFT, bool RAGGED>
void launch_phase(int phase, size_t lds, hipStream_t st, const KArgs& A) {
  with_phase(phase, [&](auto P) {
    auto kernel = sankoff_kernel<Q, SOFT, decltype(P)::value, RAGGED>;
    const int grid = phase == 1 ? persistent_grid(kernel, lds, A.nblocks) : (A.nblocks + 7) / 8 * 8;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kWave), lds, st, A);
  });
}

template <bool RAGGED>
void launch_q(int Q, int phase, bool soft, size_t lds, hipStream_t st, const KArgs& A) {
  switch (Q) {
    case 2:
      if (soft) launch_phase<2, true, RAGGED>(phase, lds, st, A);
      else launch_phase<2, false, RAGGED>(phase, lds, st, A);
      break;
    case 3:
      if (soft) launch_phase<3, true, RAGGED>(phase, lds, st, A);
      else launch_phase<3, false, RAGGED>(phase, lds, st, A);
      break;
    case 4:
      if (soft) launch_phase<4, true, RAGGED>(phase, lds, st, A);
      else launch_phase<4, false, RAGGED>(phase, lds, st, A);
      break;
  }
}

// the call record of an entry point's arguments; a ragged call passes L = 0
// and the largest tree's nl / ni, and sets rmeta / ritem / items itself
SankoffCall sankoff_call(int phase, const int* steps, const int8_t* leaves, const float* cost,
                         int B, int L, int nl, int ni, int Q, int n_slots, float tau,
                         unsigned flags, float* dp, float* site_score, float* tree_score,
                         const float* dts, float* d_cost, float* marg, int8_t* anc,
                         void* workspace, void* stream) {
  SankoffCall c;
  c.phase = phase;
  c.soft = tau > 0.0f;
  c.steps = steps;
  c.leaves = leaves;
  c.cost = cost;
  c.B = B;
  c.L = L;
  c.nl = nl;
  c.ni = ni;
  c.Q = Q;
  c.n_slots = n_slots;
  tau_coefs(tau, &c.a, &c.bcoef);
  c.hard_root = (flags & TREX_FLAG_HARD_ROOT) ? 1 : 0;
  c.dp = dp;
  c.site_score = site_score;
  c.tree_score = tree_score;
  c.dts = dts;
  c.marg = marg;
  c.anc = anc;
  c.d_cost = d_cost;
  c.workspace = workspace;
  c.stream = stream;
  return c;
}

// --------------------------------------------------------------------------
// routing: which kernel family takes a call
// --------------------------------------------------------------------------
// Q <= 4 on a small grid (few trees x few sites: C2 is one tree, 157 waves
// of 64 sites for 1 024 SIMDs) runs the state-parallel kernel instead: 4
// lanes per site (one per parent state), 16 sites per wave, 4x the waves and
// a quarter of the per-lane work on the serial node chain.
// TREX_WIDE_SMALLQ=0 / 1 forces the choice (A/B).
bool wide_small_q(int B, int L, int Q) {
  if (Q > 4) return false;
  const int forced = env_switch("TREX_WIDE_SMALLQ");
  if (forced >= 0) return forced;
  // up to ~1.5 64-site waves per CU on the lane-per-site kernel (measured
  // on 256 CUs, 32-taxa trees x 5 000 sites: 158 waves 43.8 -> 40.4 us, 316
  // waves 46.5 -> 44.9 us, 632 waves 48.2 vs 51.8 us (lane-per-site wins);
  // C2 71 -> 67 us; a C4 shard, 10 000 waves, is 2.2x slower
  // state-parallel).  Scaled by the CU count (a CPX partition has 32 CUs).
  return (int64_t)B * q4_tiles(L) * 2 <= (int64_t)3 * device_cus();
}

// Grids of at most about one state-parallel wave per SIMD (C2: one tree x
// 625 16-site items) run the staged kernel (sankoff_staged.hip): one
// workgroup of waves per item, the tree's levels spread over the waves, so
// the serial chain is the tree height instead of every internal node.
// TREX_STAGED=0 / 1 forces it off / on (whenever its LDS fits; A/B, tests).
bool use_staged(const SankoffCall& c) {
  if (staged_lds_bytes(c.ni, c.nl, c.Q, c.phase) > kLdsPerCu) return false;
  const int forced = env_switch("TREX_STAGED");
  if (forced >= 0) return forced;
  return (int64_t)c.B * wide_tiles(c.L, c.Q) <= (int64_t)4 * device_cus();
}

enum class Family { kBigq, kSite, kSite2, kStaged, kWide, kQ4, kFused4 };

struct Route {
  Family family;
  int lp_slots = -1;  // slots of the plan's lane programs (-1: a tree has none)
  // kSite / kSite2: the gate's flag and K / K^T in the wide workspace's tail,
  // and whether the fused kernel keeps its s rows (phase 3, the workspace
  // has room for them, TREX_SITE_SROW is not 0)
  int* site_flag = nullptr;
  float* site_kg = nullptr;
  bool keep_srow = false;
};

// Pure: reads the call, the plan's slot word (info[0]: stack depth |
// (lane-program slots + 1) << 16), whether the caller passed a fused Q = 4
// program, the workspace size and the TREX_* knobs (per call: the tests flip
// them inside one process).
Route route(const SankoffCall& c, int slot_word, bool has_prog, int64_t workspace_bytes) {
  Route r;
  if (c.rmeta) {
    // ragged: protein / codon alphabets on the state-parallel kernel, each
    // 64-site item split over ceil(64 / sites-per-wave) waves
    r.family = c.Q > kWideMaxQ ? Family::kBigq : c.Q > 4 ? Family::kWide : Family::kQ4;
    return r;
  }
  r.lp_slots = ((slot_word >> 16) & 0xFF) - 1;
  if (c.Q > 4 || wide_small_q(c.B, c.L, c.Q)) {
    if (c.Q > kWideMaxQ) {
      r.family = Family::kBigq;  // 64 < Q <= 128 (sankoff_bigq.hip)
    } else if (site_eligible(c, r.lp_slots)) {
      // the lane-per-site kernel (sankoff_site.hip) takes the call when the
      // cost matrix allows the factored softmin -- decided on the device: the
      // state-parallel kernel runs first, gated (every workgroup checks the
      // cost range and exits when the site kernel takes the call; workgroup
      // 0 writes K, K^T and the flag into the workspace tail), then the site
      // kernel (exits unless the flag is set), then one reduce that sums
      // whichever kernel's partials the flag names
      char* tail = static_cast<char*>(c.workspace) + wide_workspace_bytes(c.B, c.L, c.Q);
      r.site_flag = reinterpret_cast<int*>(tail - kWideTailFlag);
      r.site_kg = reinterpret_cast<float*>(tail - kWideTailKg);
      // the kept s rows are optional: a workspace without them
      // (site_srow_offset bytes) makes the adjoint recompute them
      r.keep_srow = c.phase == 3 &&
                    workspace_bytes >= trex_workspace_bytes(c.B, c.L, c.nl + c.ni, c.Q) &&
                    env_switch("TREX_SITE_SROW") != 0;
      r.family = site2_on(r.lp_slots, c.nl, c.ni) ? Family::kSite2 : Family::kSite;
    } else {
      r.family = use_staged(c) ? Family::kStaged : Family::kWide;
    }
    return r;
  }
  // the fused Q = 4 softmin kernel on the predecoded program (sankoff_fused4.hip)
  // takes the calls in its scope; same partials, same reduce
  const bool fused4 = has_prog && c.phase == 3 && c.Q == 4 && c.soft && !c.site_score &&
                      !c.marg && !c.anc && (c.L & 3) == 0 && c.nl <= kPrefetchRows &&
                      f4_lds_bytes(c.n_slots, c.nl) <= 65536 &&  // else the one-wave kernel
                      env_switch("TREX_FUSED4") != 0;
  r.family = fused4 ? Family::kFused4 : Family::kQ4;
  return r;
}

// the lane-per-site Q <= 4 kernel (prog: the fused Q = 4 one on that program),
// then the reduce of its per-item partials
int q4_run(const char* fn, const SankoffCall& c, const int32_t* prog = nullptr) {
  if ((int64_t)c.ni * c.L * c.Q * 4 > 0x7FFFFFF0LL)
    return set_error(TREX_E_UNSUPPORTED, "%s: one tree's DP table exceeds 2 GiB", fn);
  // the fused Q = 4 kernel's workgroups are kF4Waves waves on shared tables
  const size_t lds =
      prog ? f4_lds_bytes(c.n_slots, c.nl) : lds_bytes(c.n_slots, c.nl, c.Q, c.phase);
  if (lds > 65536) return set_error(TREX_E_UNSUPPORTED, "%s: LDS stack too deep", fn);
  if ((int64_t)c.B * q4_tiles(c.L) > 0x7FFFFFFF)
    return set_error(TREX_E_ARG, "%s: grid too large", fn);
  const KArgs A = q4_args(c);
  if (prog) {
    if (int e = fused4_run(fn, c, prog, lds)) return e;
  } else {
    if (!c.rmeta)
      launch_q<false>(c.Q, c.phase, c.soft, lds, (hipStream_t)c.stream, A);
    else
      launch_q<true>(c.Q, c.phase, c.soft, lds, (hipStream_t)c.stream, A);
    if (int e = hip_check(fn)) return e;
  }
  const RaggedParts rp = ragged_parts(c);
  return partial_reduce(fn, c, A.part_tree, A.part_dc, A.tiles, c.rmeta ? &rp : nullptr);
}

// common entry: validates, builds the call, routes it, launches one phase
int run_phase(const char* fn, int phase, const int32_t* plan, int n_slots, const int8_t* leaves,
              const float* cost, int B, int L, int n_all, int Q, float tau, unsigned flags,
              float* dp, float* site_score, float* tree_score, const float* dts, float* d_cost,
              float* marg, int8_t* anc, void* workspace, int64_t workspace_bytes, void* stream,
              const int32_t* prog = nullptr) {
  Shape s;
  if (int e = check_shape(fn, B, L, n_all, Q, &s)) return e;
  if (!plan || !leaves || !cost || !workspace)
    return set_error(TREX_E_ARG, "%s: null pointer argument", fn);
  if ((phase & 1) && !tree_score) return set_error(TREX_E_ARG, "%s: tree_score is required", fn);
  if ((phase & 2) && (!dp || !d_cost))
    return set_error(TREX_E_ARG, "%s: dp and d_cost are required", fn);
  if (!nonneg_finite_f32(tau))
    return set_error(TREX_E_ARG, "%s: tau must be finite and >= 0 (got %g)", fn, tau);
  // 4 < Q <= 20: the kept s rows of the fused site kernel are optional
  const int64_t min_ws = (Q > 4 && Q <= kSiteMaxQ) ? site_srow_offset(B, L, Q)
                                                   : trex_workspace_bytes(B, L, n_all, Q);
  if (workspace_bytes < min_ws) return set_error(TREX_E_ARG, "%s: workspace too small", fn);
  if (n_slots < 0) return set_error(TREX_E_ARG, "%s: bad n_slots", fn);
  if (flags & ~TREX_FLAG_HARD_ROOT) return set_error(TREX_E_ARG, "%s: unknown flags 0x%x", fn, flags);
  // n_slots is the plan's slot word: the stack depth in its low half (route)
  if ((n_slots & 0xFFFF) > 250) return set_error(TREX_E_ARG, "%s: bad n_slots", fn);
  const PlanLayout lay = plan_layout(B, s.ni);
  SankoffCall c = sankoff_call(phase, plan + lay.fwd, leaves, cost, B, L, s.nl, s.ni, Q,
                               n_slots & 0xFFFF, tau, flags, dp, site_score, tree_score, dts,
                               d_cost, marg, anc, workspace, stream);
  const Route r = route(c, n_slots, prog != nullptr, workspace_bytes);
  const int32_t* staged = plan + lay.staged;
  const int32_t* lanes = plan + lay.lanes;
  switch (r.family) {
    case Family::kBigq: return bigq_run(fn, c);
    case Family::kStaged: return staged_run(fn, c, staged);
    case Family::kWide: return wide_run(fn, c);
    case Family::kQ4: return q4_run(fn, c);
    case Family::kFused4: return q4_run(fn, c, prog);
    case Family::kSite:
    case Family::kSite2: break;
  }
  c.site_flag = r.site_flag;
  c.site_kg = r.site_kg;
  if (r.keep_srow)
    c.site_srow = reinterpret_cast<float*>(static_cast<char*>(workspace) + site_srow_offset(B, L, Q));
  if (int e = wide_run(fn, c, /*reduce=*/false)) return e;
  if (int e = r.family == Family::kSite2 ? site2_run(fn, c, lanes, r.lp_slots)
                                         : site_run(fn, c, lanes, r.lp_slots))
    return e;
  c.mx_flag = r.site_flag;
  c.mx_tiles = site_tiles(L);
  const int tiles = wide_tiles(L, Q);
  const double* part = static_cast<const double*>(workspace);
  return partial_reduce(fn, c, part, part + (int64_t)B * tiles, tiles);
}

}  // namespace

}  // namespace trex

using namespace trex;

extern "C" const char* trex_last_error(void) { return g_err; }

extern "C" int trex_version(void) { return 10; }

extern "C" int trex_dp_site_major(int Q) {
  (void)Q;
  return 1;  // every Q since v4 (Q <= 4 used [n_int][Q][L] before)
}

extern "C" int64_t trex_workspace_bytes(int B, int L, int n_all, int Q) {
  if (B <= 0 || L <= 0 || Q <= 0) return 0;
  if (Q > kWideMaxQ) return bigq_workspace_bytes(B, L, Q);
  if (Q > kSiteMaxQ) return wide_workspace_bytes(B, L, Q);
  if (Q > 4) {  // + the fused lane-per-site kernel's s rows
    const int64_t ni = tree_ni(n_all);
    return site_srow_offset(B, L, Q) + (int64_t)B * std::max<int64_t>(ni, 0) * L * Q * 4;
  }
  const int64_t nb = (int64_t)B * q4_tiles(L);
  const int64_t narrow = q4_counters_bytes(B) + nb * 8 * (1 + (int64_t)Q * Q) + (int64_t)Q * Q * B * 8 + 256;
  // small grids may run the state-parallel wide kernel (G = 4): room for both
  return std::max<int64_t>(narrow, wide_workspace_bytes(B, L, Q));
}

extern "C" int trex_workspace_init(void* workspace, int64_t workspace_bytes, void* stream) {
  if (!workspace || workspace_bytes <= 0)
    return set_error(TREX_E_ARG, "trex_workspace_init: bad arguments");
  if (hipMemsetAsync(workspace, 0, (size_t)workspace_bytes, (hipStream_t)stream) != hipSuccess)
    return hip_check("trex_workspace_init");
  return hip_check("trex_workspace_init");
}

extern "C" int trex_sankoff_fwd(const int32_t* plan, int n_slots, const int8_t* leaves,
                                const float* cost, int B, int L, int n_all, int Q, float tau,
                                unsigned flags, float* dp, float* site_score, float* tree_score,
                                void* workspace, int64_t workspace_bytes, void* stream) {
  if (!dp)
    return set_error(TREX_E_UNSUPPORTED,
                     "trex_sankoff_fwd: dp is required (the reference returns the table)");
  return run_phase("trex_sankoff_fwd", 1, plan, n_slots, leaves, cost, B, L, n_all, Q, tau, flags,
                   dp, site_score, tree_score, nullptr, nullptr, nullptr, nullptr, workspace,
                   workspace_bytes, stream);
}

extern "C" int trex_sankoff_bwd(const int32_t* plan, int n_slots, const int8_t* leaves,
                                const float* cost, int B, int L, int n_all, int Q, float tau,
                                unsigned flags, const float* dp, const float* d_tree_score,
                                float* d_cost, float* marginals, int8_t* anc_states,
                                void* workspace, int64_t workspace_bytes, void* stream) {
  return run_phase("trex_sankoff_bwd", 2, plan, n_slots, leaves, cost, B, L, n_all, Q, tau, flags,
                   const_cast<float*>(dp), nullptr, nullptr, d_tree_score, d_cost, marginals,
                   anc_states, workspace, workspace_bytes, stream);
}

extern "C" int trex_sankoff_fwd_bwd(const int32_t* plan, int n_slots, const int8_t* leaves,
                                    const float* cost, int B, int L, int n_all, int Q, float tau,
                                    unsigned flags, float* dp, float* site_score,
                                    float* tree_score, const float* d_tree_score, float* d_cost,
                                    float* marginals, int8_t* anc_states, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  return run_phase("trex_sankoff_fwd_bwd", 3, plan, n_slots, leaves, cost, B, L, n_all, Q, tau,
                   flags, dp, site_score, tree_score, d_tree_score, d_cost, marginals, anc_states,
                   workspace, workspace_bytes, stream);
}

extern "C" int trex_sankoff_fwd_bwd_prog(const int32_t* plan, int n_slots, const int8_t* leaves,
                                         const float* cost, int B, int L, int n_all, int Q,
                                         float tau, unsigned flags, float* dp, float* site_score,
                                         float* tree_score, const float* d_tree_score,
                                         float* d_cost, float* marginals, int8_t* anc_states,
                                         void* workspace, int64_t workspace_bytes, void* stream,
                                         const int32_t* prog) {
  return run_phase("trex_sankoff_fwd_bwd_prog", 3, plan, n_slots, leaves, cost, B, L, n_all, Q,
                   tau, flags, dp, site_score, tree_score, d_tree_score, d_cost, marginals,
                   anc_states, workspace, workspace_bytes, stream, prog);
}

extern "C" int trex_sankoff_backtrack(const int32_t* plan, int backtrack_ok, const float* cost,
                                      const float* dp, int B, int L, int n_all, int Q,
                                      int8_t* anc_states, void* stream) {
  Shape s;
  if (int e = check_shape("trex_sankoff_backtrack", B, L, n_all, Q, &s)) return e;
  if (!backtrack_ok)
    return set_error(TREX_E_TOPOLOGY,
                     "trex_sankoff_backtrack: the reference backtrack does not terminate on this "
                     "topology (cyclic child references)");
  if (!plan || !cost || !dp || !anc_states)
    return set_error(TREX_E_ARG, "trex_sankoff_backtrack: null pointer argument");
  const int32_t* bt32 = plan + plan_layout(B, s.ni).bt;
  if (Q > kWideMaxQ) return bigq_backtrack(bt32, cost, dp, B, L, s.ni, Q, anc_states, stream);
  // every uniform batch: the split-lane kernels of sankoff_wide.hip (4 lanes
  // per site for Q <= 4, 8 for Q <= 32, one lane per site for codons); ragged
  // Q <= 4 batches have their own kernel (trex_sankoff_ragged_backtrack)
  return wide_backtrack(bt32, cost, dp, B, L, s.ni, Q, anc_states, stream);
}

extern "C" int trex_dp_to_trex_layout(const float* dp, const int8_t* leaves, int B, int L,
                                      int n_all, int Q, float* out, void* stream) {
  if (B <= 0 || L <= 0 || n_all < 3 || Q < 2 || Q > kBigMaxQ || !dp || !leaves || !out)
    return set_error(TREX_E_ARG, "trex_dp_to_trex_layout: bad arguments");
  const int nl = tree_nl(n_all);
  const size_t total = (size_t)B * n_all * L;
  const int grid = (int)std::min<size_t>((total + 255) / 256, 65536);
  hipLaunchKernelGGL(to_trex_layout_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, dp,
                     leaves, B, L, n_all, nl, Q, out);
  return hip_check("trex_dp_to_trex_layout");
}

// ---------------------------------------------------------------------------
// Ragged batches (trees of different n_all / L in one launch; plan from
// trex_ragged_plan_build).  Packed layouts: leaves [sum n_leaves_b * L_b]
// int8 (tree b at its leaf offset, [n_leaves_b][L_b]); dp / marginals
// [sum n_int_b * L_b][Q] f32 (tree b: [n_int_b][L_b][Q]); site_score
// [sum L_b]; anc_states [sum n_int_b * L_b] int8.
// ---------------------------------------------------------------------------
extern "C" int64_t trex_ragged_workspace_bytes(int64_t items, int Q) {
  if (items <= 0 || Q <= 0) return 0;
  if (Q > kWideMaxQ) return items * 8 * (1 + (int64_t)Q * Q) + 256;  // partials per item
  if (Q > 4) return wide_ragged_workspace_bytes(items, Q);  // partials per wave
  return items * 8 * (1 + (int64_t)Q * Q) + 256;
}

extern "C" int trex_sankoff_ragged(int phase, const int32_t* plan, int B, int n_slots, int max_nl,
                                   int64_t items, const int8_t* leaves, const float* cost, int Q,
                                   float tau, unsigned flags, float* dp, float* site_score,
                                   float* tree_score, const float* d_tree_score, float* d_cost,
                                   float* marginals, int8_t* anc_states, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  const char* fn = "trex_sankoff_ragged";
  if (phase < 1 || phase > 3) return set_error(TREX_E_ARG, "%s: phase must be 1, 2 or 3", fn);
  if (B <= 0 || items <= 0 || items > 0x7FFFFFFF || max_nl < 2 || Q < 2)
    return set_error(TREX_E_ARG, "%s: bad shape B=%d items=%lld max_nl=%d Q=%d", fn, B,
                     (long long)items, max_nl, Q);
  if (Q > kBigMaxQ)
    return set_error(TREX_E_UNSUPPORTED, "%s: Q=%d > %d not supported by this build (int8 leaf "
                     "codes / ancestral states)", fn, Q, kBigMaxQ);
  if (!plan || !leaves || !cost || !workspace || !dp)
    return set_error(TREX_E_ARG, "%s: null pointer argument", fn);
  if ((phase & 1) && !tree_score) return set_error(TREX_E_ARG, "%s: tree_score is required", fn);
  if ((phase & 2) && !d_cost) return set_error(TREX_E_ARG, "%s: d_cost is required", fn);
  if (!nonneg_finite_f32(tau))
    return set_error(TREX_E_ARG, "%s: tau must be finite and >= 0 (got %g)", fn, tau);
  if (workspace_bytes < trex_ragged_workspace_bytes(items, Q))
    return set_error(TREX_E_ARG, "%s: workspace too small", fn);
  if (n_slots < 0 || n_slots > 250) return set_error(TREX_E_ARG, "%s: bad n_slots", fn);
  if (flags & ~TREX_FLAG_HARD_ROOT) return set_error(TREX_E_ARG, "%s: unknown flags 0x%x", fn, flags);
  // the plan: per-tree records, the work-item -> tree table, the steps
  const RaggedLayout lay = ragged_layout(B, items, 0);
  const int* meta = plan + lay.meta;
  const int* ritem = plan + lay.item;
  SankoffCall c = sankoff_call(phase, plan + lay.fwd, leaves, cost, B, 0, max_nl, max_nl - 1, Q,
                               n_slots, tau, flags, dp, site_score, tree_score, d_tree_score,
                               d_cost, marginals, anc_states, workspace, stream);
  c.rmeta = meta;
  c.ritem = ritem;
  c.items = items;
  switch (route(c, n_slots, false, workspace_bytes).family) {
    case Family::kBigq: return bigq_run(fn, c);
    case Family::kWide: return wide_ragged_run(fn, c);
    default: return q4_run(fn, c);
  }
}

extern "C" int trex_sankoff_ragged_backtrack(const int32_t* plan, int B, int64_t items,
                                             int64_t steps, int backtrack_ok, const float* cost,
                                             const float* dp, int Q, int8_t* anc_states,
                                             void* stream) {
  const char* fn = "trex_sankoff_ragged_backtrack";
  if (B <= 0 || items <= 0 || items > 0x7FFFFFFF || steps <= 0 || Q < 2)
    return set_error(TREX_E_ARG, "%s: bad arguments", fn);
  if (Q > kBigMaxQ)
    return set_error(TREX_E_UNSUPPORTED, "%s: Q=%d > %d not supported by this build", fn, Q,
                     kBigMaxQ);
  if (!backtrack_ok)
    return set_error(TREX_E_TOPOLOGY,
                     "%s: the reference backtrack does not terminate on this batch (cyclic child "
                     "references)", fn);
  if (!plan || !cost || !dp || !anc_states) return set_error(TREX_E_ARG, "%s: null pointer", fn);
  const int* meta = plan + ragged_layout(B, items, steps).meta;
  if (Q > kWideMaxQ) return bigq_ragged_backtrack(meta, B, items, steps, cost, dp, Q, anc_states, stream);
  if (Q > 4) return wide_ragged_backtrack(meta, B, items, steps, cost, dp, Q, anc_states, stream);
  hipStream_t st = (hipStream_t)stream;
#define TREX_RBT(QQ)                                                                            \
  hipLaunchKernelGGL(sankoff_ragged_backtrack_kernel<QQ>, dim3((int)items), dim3(kWave), 0, st, \
                     meta, cost, dp, anc_states, B, (int)items, (int)steps);
  switch (Q) {
    case 2: TREX_RBT(2) break;
    case 3: TREX_RBT(3) break;
    case 4: TREX_RBT(4) break;
  }
#undef TREX_RBT
  return hip_check(fn);
}
