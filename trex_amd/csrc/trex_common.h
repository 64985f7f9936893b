// Shared constants and error plumbing for libtrexhip.so (host side).
#pragma once

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "../../include/trex_hip.h"

namespace trex {

// word 0 of the header of everything plan.cpp builds
constexpr int32_t kPlanMagic = 0x54524558;    // 'TREX' trex_plan_build
constexpr int32_t kF4Magic = 0x54524634;      // 'TRF4' trex_fused4_program_build
constexpr int32_t kRaggedMagic = 0x54525247;  // 'TRRG' trex_ragged_plan_build
constexpr int32_t kNniMagic = 0x54524E4E;     // 'TRNN' trex_nni_plan_build
constexpr int32_t kAttachMagic = 0x54524154;  // 'TRAT' trex_attach_plan_build
constexpr int32_t kSprMagic = 0x54525350;     // 'TRSP' trex_spr_plan_build
// SPR plan, ints per tree: node records [n_all][4] | walk records [n_int][4]
inline int64_t spr_tree_ints(int ni) { return 12LL * ni + 4; }
constexpr size_t kLdsPerCu = 160 * 1024;    // gfx950: LDS bytes of a CU, the most one workgroup can take

// leaves / internal rows of a tree of n_all nodes
inline int tree_nl(int n_all) { return (n_all + 1) / 2; }
inline int tree_ni(int n_all) { return n_all - tree_nl(n_all); }

// forward-step child descriptor: index bits 0-15, slot 16-23, kind 24-25,
// flags above.  Kinds: a row that still holds the 1e5 init (index 0), a leaf
// (leaf index), an internal row (row, and the LDS slot its vector is in), a
// row the lane-per-site program computes inline (its index in the inline list)
constexpr int kKindSent = 0, kKindLeaf = 1, kKindInt = 2, kKindInline = 3;
inline int32_t child_desc(int kind, int index, int slot = 0, int32_t flags = 0) {
  return (index & 0xFFFF) | ((slot & 0xFF) << 16) | (kind << 24) | flags;
}
// node id -> leaf or internal-row descriptor (NNI and attach plans)
inline int32_t node_desc(int node, int nl) {
  return node < nl ? child_desc(kKindLeaf, node) : child_desc(kKindInt, node - nl);
}
inline int desc_index(int32_t d) { return d & 0xFFFF; }
inline int desc_slot(int32_t d) { return (d >> 16) & 0xFF; }
inline int desc_kind(int32_t d) { return (d >> 24) & 3; }
// word 0 of a step: the row it computes, the slot its vector goes to
inline int32_t step_row(int row, int slot = 0) { return child_desc(0, row, slot); }
constexpr int32_t kStepAccumulate = 1 << 26;  // adjoint: add into the slot
// register bypass: this internal child is the previous step's node (its only
// consumer is this step): forward reads its D from registers, the adjoint
// hands its cotangent to the next reverse step in registers
constexpr int32_t kChildPrev = 1 << 27;
// deferred edge (Q <= 4 adjoint; other kernels ignore it): this internal
// child is a cherry (both of its children leaves / 1e5 rows) with one
// parent.  The parent's step hands its own cotangent to the child's slot
// (or the bypass) instead of the child's, reading no DP row; the child's step
// (kStepDeferredIn) recomputes its D from its leaf messages (or looks the
// edge's weights up by its two leaf codes, sankoff.hip pair tables) and runs
// the edge adjoint first.  A cherry's row is then never re-read from HBM.
constexpr int32_t kChildDeferred = 1 << 28;
// forward-step flags (word 3)
constexpr int32_t kStepRoot = 1;
constexpr int32_t kStepUnreached = 2;
constexpr int32_t kStepToNext = 4;  // output consumed only by the next step (bypass)
constexpr int32_t kStepDeferredIn = 8;  // slot / bypass holds the parent's cotangent

// Staged (multi-wave) program, after the backtrack entries of a plan: one
// region of staged_tree_ints(ni) ints per tree, steps [ni][4] (same words as
// the forward steps; every internal row has its own LDS slot = its row, so
// no slot / bypass fields) | S (stages) | offsets [S * kStageWaves + 1]:
// steps of stage s on wave w are [off[s*W + w], off[s*W + w + 1]).  The
// waves of one workgroup run a stage's node lists in parallel, a barrier
// between stages (sankoff_staged.hip).
constexpr int kStageWaves = 8;
inline int64_t staged_tree_ints(int ni) {
  return 4LL * ni + (((int64_t)ni * kStageWaves + 2 + 3) & ~3LL);
}

// Lane-per-site program (sankoff_site.hip), after the staged regions: one
// region of lp_tree_ints(ni) ints per tree (plan.cpp lane_program_one_tree):
//   [0] S (stages)  [1] n_slots (-1: the tree cannot run it)  [2] n_steps
//   [3] n_inline  [4 .. 4 + S] stage offsets: stage s = steps [off[s], off[s+1])
//   steps at lp_steps_offset(ni): [n_steps][4] = {row | slot << 16,
//     child desc 0, child desc 1, flags (kStepRoot)}, then the inline rows
//     [n_inline][4] = {row, child desc 0, child desc 1, height}, children first.
//   child desc: kind << 24 | (sentinel: 0; leaf: leaf index; task row:
//     row | slot << 16 (kKindInt); inline row: its index (kKindInline))
inline int64_t lp_steps_offset(int ni) { return 8 + (((int64_t)ni + 1 + 3) & ~3LL); }
inline int64_t lp_tree_ints(int ni) { return lp_steps_offset(ni) + 4LL * ni; }

// Where a uniform plan's regions start, in ints from the plan's first:
// header | fwd steps [B][ni][4] | backtrack entries [B][ni][2] | staged
// regions [B] | lane-per-site regions [B].  The writer (plan.cpp) and the
// readers (sankoff.hip) both take their pointers from here.
struct PlanLayout {
  int64_t fwd, bt, staged, lanes, total;
};
inline PlanLayout plan_layout(int B, int ni) {
  const int64_t fwd = TREX_PLAN_HEADER_INTS, bt = fwd + (int64_t)B * ni * 4,
                staged = bt + (int64_t)B * ni * 2, lanes = staged + B * staged_tree_ints(ni);
  return {fwd, bt, staged, lanes, lanes + B * lp_tree_ints(ni)};
}

// A ragged plan (trees of different sizes n_all_b and site counts L_b in one
// launch; one work item = one tree x 64-site tile): header | per-tree records
// [B][kRaggedMeta] | work item -> tree [items] | fwd steps [steps][4] |
// backtrack entries [steps][2], steps = sum n_int_b.  The kernels index the
// plan from its records on (rmeta) by the same sums.
constexpr int kRaggedMeta = 12;  // ints per tree record, the last two spare
enum RaggedRecord {
  kRecStep = 0,  // the tree's first step
  kRecNInt,
  kRecNLeaves,
  kRecL,
  kRecSite,    // its first site in the packed site arrays
  kRecItem,    // its first work item
  kRecLeafLo,  // its offset in the packed leaf bytes (64 bits)
  kRecLeafHi,
  kRecRowsLo,  // its offset in the packed DP row-sites (64 bits)
  kRecRowsHi,
};
struct RaggedLayout {
  int64_t meta, item, fwd, bt, total;
};
// a reader that stops at the steps may pass steps = 0
inline RaggedLayout ragged_layout(int B, int64_t items, int64_t steps) {
  const int64_t meta = TREX_PLAN_HEADER_INTS, item = meta + (int64_t)B * kRaggedMeta,
                fwd = item + items, bt = fwd + steps * 4;
  return {meta, item, fwd, bt, bt + steps * 2};
}

// Fused Q = 4 program (trex_fused4_program_build, plan.cpp; run by
// sankoff_fused4.hip): the plan's forward steps decoded once on the host, so
// the kernel's loops read operands instead of decoding descriptors.  Layout
// (ints): header [TREX_PLAN_HEADER_INTS] = {kF4Magic, B, n_all, n_int, 0...}
// | records [B][n_int][kF4RecInts], tree by tree in the plan's step order.
// Record (32 bytes, one scalar load):
//   [0] flags: the kF4* bits below | forward class << 16
//   [1] DP row of the step's node
//   [2] [3] operand of child 0 / child 1 (stored order), an LDS byte offset:
//       leaf child: leaf index * 64 into the leaf tile (+ lane);
//       internal child: slot * 1024 into the slot stack (+ lane * 16), 0 when
//       the child is the previous step (kF4Prev*, register bypass)
//   [4] the node's own slot * 1024 (forward sink when kF4Put, reverse
//       cotangent source unless kF4ToNext / kF4Root); 0 when it has none
//   [5] [6] DP row of child 0 / child 1 that the adjoint re-reads, or
//       kF4NoRow (leaf child, deferred cherry: nothing is read)
//   [7] 0
// Forward classes: kF4Cherry both children leaves; kF4CherryDeferred the same
// with the parent edge deferred to this step (kStepDeferredIn: pair tables);
// kF4LeafInt one leaf and one internal child (kF4Leaf0 tells which: the sum
// of the two messages commutes); kF4IntInt.  The reverse sweep runs the
// children in stored order off the flag bits (the dC sums depend on the order).
constexpr int kF4RecInts = 8;
constexpr int32_t kF4Leaf0 = 1, kF4Leaf1 = 2;    // child 0 / 1 is a leaf
constexpr int32_t kF4Prev0 = 4, kF4Prev1 = 8;    // kChildPrev of child 0 / 1
constexpr int32_t kF4Defer0 = 16, kF4Defer1 = 32;  // kChildDeferred of child 0 / 1
constexpr int32_t kF4DeferIn = 64;               // kStepDeferredIn
constexpr int32_t kF4ToNext = 128;               // kStepToNext
constexpr int32_t kF4Root = 256;                 // kStepRoot
constexpr int32_t kF4Put = 512;                  // the forward writes the node's slot
constexpr int kF4Cherry = 0, kF4CherryDeferred = 1, kF4LeafInt = 2, kF4IntInt = 3;
constexpr int kF4FwdClassShift = 16;
constexpr int32_t kF4NoRow = -1;
// backtrack entry kinds (bits 16-19 of word 0)
constexpr int kBtRoot = 0;
constexpr int kBtReal = 1;
constexpr int kBtSentinel = 2;
constexpr int kBtUnreached = 3;

int set_error(int code, const char* fmt, ...);
// TREX_OK, or TREX_E_HIP with the pending HIP error's text as the last error
int hip_check(const char* fn);
// softmin coefficients of a temperature: a = log2(e) / tau, bcoef = tau ln 2
// (exp(-x / tau) = exp2(-x a), tau ln(s) = bcoef log2(s)); 0, 0 for tau = 0
void tau_coefs(float tau, float* a, float* bcoef);

// Host argument checks on the IEEE bit pattern: the library is compiled with
// -fno-honor-nans (kernels drop NaN canonicalisation), under which the
// compiler may fold `!(x >= 0.0f)` or std::isnan(x) to false for a NaN x.
inline uint32_t float_bits(float x) {
  uint32_t u;
  std::memcpy(&u, &x, sizeof u);
  return u;
}
inline bool finite_f32(float x) { return (float_bits(x) & 0x7f800000u) != 0x7f800000u; }
// finite and >= 0 (-0.0 included)
inline bool nonneg_finite_f32(float x) {
  const uint32_t u = float_bits(x);
  return finite_f32(x) && (!(u >> 31) || (u & 0x7fffffffu) == 0);
}
// finite and > 0
inline bool pos_finite_f32(float x) {
  const uint32_t u = float_bits(x);
  return finite_f32(x) && !(u >> 31) && (u & 0x7fffffffu) != 0;
}

// 1 / 0 from the first character of an on / off knob, -1 when it is unset or
// anything else.  Read per call: the tests flip the knobs inside one process.
// "TREX_X=0 / 1 forces" reads as >= 0, "off when 0" as != 0.
inline int env_switch(const char* name) {
  const char* e = std::getenv(name);
  return e && (e[0] == '0' || e[0] == '1') ? e[0] - '0' : -1;
}

// a run-time phase (1 fwd, 2 adjoint, 3 fused) as a compile-time one:
// f(std::integral_constant<int, PHASE>())
template <class F>
void with_phase(int phase, F&& f) {
  if (phase == 1)
    f(std::integral_constant<int, 1>());
  else if (phase == 2)
    f(std::integral_constant<int, 2>());
  else
    f(std::integral_constant<int, 3>());
}

// ---- one Sankoff call, uniform or ragged, at any Q: the entry point's
// arguments as every kernel family's host code takes them (sankoff_call,
// sankoff.hip).  A ragged call has L = 0, the largest tree's nl / ni, and the
// plan's records in rmeta / ritem / items.
struct SankoffCall {
  int phase;  // 1 fwd, 2 adjoint, 3 fused
  bool soft;
  const int* steps;
  const int8_t* leaves;
  const float* cost;
  int B, L, nl, ni, Q, n_slots;
  float a, bcoef;
  int hard_root;
  float* dp;
  float* site_score;
  float* tree_score;
  const float* dts;
  float* marg;
  int8_t* anc;
  float* d_cost;
  void* workspace;
  void* stream;
  // ragged batches (null / 0 for uniform ones): per-tree records, the
  // work-item -> tree table, the number of 64-site items
  const int* rmeta = nullptr;
  const int* ritem = nullptr;
  int64_t items = 0;
  // set when the lane-per-site kernel (sankoff_site.hip) ran first: the device
  // word it wrote (1: it handled the launch -- the state-parallel kernels
  // exit at once, the reduce sums its mx_tiles partials per tree)
  const int* mx_flag = nullptr;
  int mx_tiles = 0;
  // gated launch (run_phase): the state-parallel kernel decides per
  // workgroup whether the lane-per-site kernel takes the call and writes
  // its K / K^T (site_kg) and the flag (site_flag) from workgroup 0
  int* site_flag = nullptr;
  float* site_kg = nullptr;
  // fused site kernel: its forward's softmin row sums s = K u of every
  // internal child row it computes, re-read by its adjoint (workspace past
  // the wide workspace, DP-table layout; null: recomputed)
  float* site_srow = nullptr;
};

// The fields every kernel argument struct (KArgs, WArgs, SArgs, SiteArgs,
// Site2Args, BigArgs) shares, from a call: a uniform batch of B trees of
// n_int rows, L sites and tiles items each, or (n_int = L = tiles = 0) a
// ragged one.  The partials sit part_offset bytes into the workspace: nitems
// per-item scores, then the [Q*Q][nitems] dC partials.  The launcher sets
// what is its own.
template <class Args>
void fill_common(Args& A, const SankoffCall& c, int n_int, int L, int tiles, int64_t nitems,
                 int64_t part_offset = 0) {
  A.leaves = c.leaves;
  A.cost = c.cost;
  A.n_int = n_int;
  A.nl = c.nl;
  A.L = L;
  A.tiles = tiles;
  A.B = c.B;
  A.a = c.a;
  A.bcoef = c.bcoef;
  A.hard_root = c.hard_root;
  A.dp = c.dp;
  A.site_score = c.site_score;
  A.dts = c.dts;
  A.marg = c.marg;
  A.anc = c.anc;
  A.part_tree = reinterpret_cast<double*>(static_cast<char*>(c.workspace) + part_offset);
  A.part_dc = A.part_tree + nitems;
}

// the fused Q = 4 kernel (sankoff_fused4.hip) on a call run_phase found in
// scope; prog: the device copy of the program
int fused4_run(const char* fn, const SankoffCall& c, const int32_t* prog, size_t lds);

// ---- Q > 4: state-parallel kernels on a site-major DP table (sankoff_wide.hip)
constexpr int kWideMaxQ = 64;
// 64 < Q <= 128: the large-alphabet kernel (sankoff_bigq.hip; int8 leaf codes
// and ancestral states bound Q by 128)
constexpr int kBigMaxQ = 128;
int bigq_tiles(int L);
int64_t bigq_workspace_bytes(int B, int L, int Q);
int bigq_run(const char* fn, const SankoffCall& c);  // uniform or ragged
int bigq_backtrack(const int32_t* bt, const float* cost, const float* dp, int B, int L, int ni,
                   int Q, int8_t* anc, void* stream);
int bigq_ragged_backtrack(const int32_t* rmeta, int B, int64_t items, int64_t steps,
                          const float* cost, const float* dp, int Q, int8_t* anc, void* stream);
int wide_group(int Q);
int wide_tiles(int L, int Q);
size_t wide_lds_bytes(int n_slots, int nl, int ni, int Q);
// per-item partials, then a tail (from its end): the site gate's flag (128 B),
// below it K and K^T of the lane-per-site kernel (3.25 KB), its cherry tables
// and the staged kernel's counter
int64_t wide_workspace_bytes(int B, int L, int Q);
constexpr int kWideTailFlag = 128;  // the flag sits this far below the end
constexpr int kWideTailKg = 3456;   // and K, K^T this far
int wide_run(const char* fn, const SankoffCall& c, bool reduce = true);
// staged multi-wave kernel (sankoff_staged.hip); staged = the plan's staged
// regions (after the backtrack entries)
size_t staged_lds_bytes(int ni, int nl, int Q, int phase);
int staged_run(const char* fn, const SankoffCall& c, const int32_t* staged);
// a ragged batch's partials: first[b * stride] is tree b's first item, items
// the total, scale the partials per item (the wide kernel's waves per item)
struct RaggedParts {
  const int* first;
  int stride, items, scale;
};
inline RaggedParts ragged_parts(const SankoffCall& c, int scale = 1) {
  return {c.rmeta + kRecItem, kRaggedMeta, (int)c.items, scale};
}
// fixed-order sum of per-item partials -> c.tree_score [B] (phase & 1),
// c.d_cost [Q*Q] (phase & 2); part_dc is [Q*Q][B*tiles] (ragged: tiles is
// unused).  When *c.mx_flag is set on the device, the partials are the
// lane-per-site kernel's, c.mx_tiles per tree.
int partial_reduce(const char* fn, const SankoffCall& c, const double* part_tree,
                   const double* part_dc, int tiles, const RaggedParts* ragged = nullptr);
// ragged batches with Q > 4 on the wide kernel (c.nl = max leaves)
int64_t wide_ragged_workspace_bytes(int64_t items, int Q);
int wide_ragged_run(const char* fn, const SankoffCall& c);
// lane-per-site kernel for the factored softmin, 4 < Q <= 20 (sankoff_site.hip)
bool site_eligible(const SankoffCall& c, int lp_slots);
constexpr int kSiteMaxQ = 20;  // the lane-per-site kernel's largest Q (kSiteSQ, wide_dev.h)
inline int64_t site_srow_offset(int B, int L, int Q) {
  return (wide_workspace_bytes(B, L, Q) + 255) / 256 * 256;
}
int site_tiles(int L);
// behind a gated wide_run: c.site_flag / c.site_kg are what that wrote
int site_run(const char* fn, const SankoffCall& c, const int32_t* lanes, int lp_slots);
// the same with each site's states split over a wave pair (sankoff_site2.hip;
// TREX_SITE2=1 / 8 / 6 / 4, read per call: the pair count, when its LDS fits)
bool site2_on(int lp_slots, int nl, int ni);
int site2_run(const char* fn, const SankoffCall& c, const int32_t* lanes, int lp_slots);
int wide_backtrack(const int32_t* bt, const float* cost, const float* dp, int B, int L, int ni,
                   int Q, int8_t* anc, void* stream);
int wide_ragged_backtrack(const int32_t* rmeta, int B, int64_t items, int64_t steps,
                          const float* cost, const float* dp, int Q, int8_t* anc, void* stream);

}  // namespace trex
