// Host-side topology planner for libtrexhip.so.
//
// Turns trex's per-node child lists (jnp.where(adj[:, node] == 1, size=2,
// fill_value=-1), src/trex/sankoff.py:60) into a per-tree "program" the HIP
// kernels execute with wave-uniform control flow:
//
//  * forward steps in a post-order that evaluates the child needing more
//    stack slots first (Sethi-Ullman), so live internal DP vectors fit a
//    log2(n)+1-deep per-lane LDS stack instead of being re-read from HBM;
//  * the child rules of trex's run_dp: c == -1 or c >= node reads a row that
//    still holds the 1e5 init (sankoff.py:60,67,152), c < n_leaves is a leaf,
//    otherwise an already computed internal row;
//  * adjoint flags for the reverse sweep (which reverse step first writes a
//    child's cotangent slot, which nodes the root never reaches);
//  * the reference backtrack's visiting order (sankoff.py:212-265), simulated
//    once on the topology (the DFS node sequence does not depend on states),
//    reduced to "node x takes its state from parent p at x's last visit".
//
// This is integer work on B * n_all entries, done once per topology (the
// reference re-traces per static shape, sankoff.py:114).  Every tree is
// analysed once (analyse_tree -> TreeShape); the program builders
// (plan_one_tree, stage_one_tree, lane_program_one_tree) read that record.  Child
// descriptors and the region layouts come from trex_common.h.
#include <algorithm>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <queue>
#include <set>
#include <vector>

#include "trex_common.h"

namespace trex {

namespace {

struct Child {
  int kind;
  int index;  // leaf index or internal row
};

// One tree's child lists under the child rules above, and what follows from
// them alone.  Rows are the internal nodes, row r = node nl + r; a "real"
// child of a row is an internal row it reads (kKindInt).
struct TreeShape {
  const int32_t* ch;  // the raw child lists [n_all][2]
  int n_all, nl, ni;
  std::vector<Child> kids;   // [ni][2]
  std::vector<int> refs;     // how many rows list row r as a real child
  std::vector<int> parent;   // the last of them (its one parent in a tree), -1: none
  std::vector<int> height;   // 1 + the tallest real child's (no real child: 1)
  std::vector<char> reach;   // the root reaches row r along real edges
  int n_dag, n_unreached;    // rows with refs > 1 / rows the root does not reach
  const Child& kid(int r, int k) const { return kids[2 * r + k]; }
};

// false on a malformed child id; t is reused from tree to tree
bool analyse_tree(const int32_t* ch, int n_all, TreeShape& t) {
  const int nl = tree_nl(n_all), ni = n_all - nl;
  t.ch = ch;
  t.n_all = n_all;
  t.nl = nl;
  t.ni = ni;
  t.kids.resize(2 * ni);
  t.refs.assign(ni, 0);
  t.parent.assign(ni, -1);
  t.height.assign(ni, 1);
  for (int r = 0; r < ni; ++r) {
    const int node = nl + r;
    for (int k = 0; k < 2; ++k) {
      const int c = ch[2 * node + k];
      if (c < -1 || c >= n_all) return false;
      Child cd = {kKindSent, 0};  // c == -1 or c >= node: a row that still holds the 1e5 init
      if (c != -1 && c < node && c < nl) {
        cd = {kKindLeaf, c};
      } else if (c != -1 && c < node) {
        cd = {kKindInt, c - nl};
        t.refs[c - nl] += 1;
        t.parent[c - nl] = r;
        t.height[r] = std::max(t.height[r], t.height[c - nl] + 1);
      }
      t.kids[2 * r + k] = cd;
    }
  }
  t.reach.assign(ni, 0);
  t.reach[ni - 1] = 1;
  for (int r = ni - 1; r >= 0; --r) {
    if (!t.reach[r]) continue;
    for (int k = 0; k < 2; ++k)
      if (t.kid(r, k).kind == kKindInt) t.reach[t.kid(r, k).index] = 1;
  }
  t.n_dag = t.n_unreached = 0;
  for (int r = 0; r < ni; ++r) {
    t.n_dag += t.refs[r] > 1;
    t.n_unreached += !t.reach[r];
  }
  return true;
}

// offs[0 .. n_buckets] over n steps sorted by bucket: bucket j is the steps
// [offs[j], offs[j + 1])
template <class BucketOf>
void bucket_offsets(int32_t* offs, int n_buckets, int n, BucketOf bucket_of) {
  for (int j = 0; j <= n_buckets; ++j) offs[j] = n;
  for (int k = n - 1; k >= 0; --k) offs[bucket_of(k)] = k;
  for (int j = n_buckets - 1; j >= 0; --j) offs[j] = std::min(offs[j], offs[j + 1]);
}

// a header: zeros, the magic, then the fields from word 1 on
void write_header(int32_t* plan, int32_t magic, std::initializer_list<int32_t> fields) {
  std::memset(plan, 0, sizeof(int32_t) * TREX_PLAN_HEADER_INTS);
  plan[0] = magic;
  std::copy(fields.begin(), fields.end(), plan + 1);
}

// the shapes every builder but trex_ragged_plan_build takes (16-bit row ids)
bool uniform_shape(int B, int n_all) { return B > 0 && n_all >= 3 && n_all <= 65535; }

// TREX_DEFER=0 turns the deferred cherry edges off (A/B, tests); read per
// plan build, so one process can build both kinds
bool defer_enabled() {
  const char* e = std::getenv("TREX_DEFER");
  return !(e && e[0] == '0');
}

// Forward steps and backtrack entries of one tree.  Returns false when the
// schedule misses a row or does not end at the root, or needs more than 250
// slots.
bool plan_one_tree(const TreeShape& t, bool defer_on, int32_t* fwd, int32_t* bt, int* n_slots,
                   int* bt_ok) {
  const int nl = t.nl, ni = t.ni;
  const std::vector<int>& refs = t.refs;
  // Sethi-Ullman need, rows in increasing order (internal children are lower)
  std::vector<int> need(ni, 1);
  for (int r = 0; r < ni; ++r) {
    int a = 0, b = 0;
    for (int k = 0; k < 2; ++k) {
      const Child& cd = t.kid(r, k);
      if (cd.kind == kKindInt) {
        const int n = need[cd.index];
        if (n > a) { b = a; a = n; } else if (n > b) { b = n; }
      }
    }
    need[r] = std::max({1, a, b + 1});
  }

  // schedule: post-order DFS, heavier child first; orphans first, root last
  std::vector<int> order;
  order.reserve(ni);
  std::vector<char> done(ni, 0);
  auto visit = [&](int start) {
    std::vector<std::pair<int, int>> st;  // (row, phase)
    st.push_back({start, 0});
    while (!st.empty()) {
      auto [r, ph] = st.back();
      st.pop_back();
      if (done[r]) continue;
      if (ph == 1) {
        done[r] = 1;
        order.push_back(r);
        continue;
      }
      st.push_back({r, 1});
      int c0 = -1, c1 = -1;
      if (t.kid(r, 0).kind == kKindInt) c0 = t.kid(r, 0).index;
      if (t.kid(r, 1).kind == kKindInt) c1 = t.kid(r, 1).index;
      // push the lighter first so the heavier is evaluated first
      int heavy = c0, light = c1;
      if (c0 < 0 || (c1 >= 0 && need[c1] > need[c0])) { heavy = c1; light = c0; }
      if (light >= 0 && !done[light]) st.push_back({light, 0});
      if (heavy >= 0 && !done[heavy]) st.push_back({heavy, 0});
    }
  };
  for (int r = 0; r < ni - 1; ++r)
    if (refs[r] == 0) visit(r);
  visit(ni - 1);
  if ((int)order.size() != ni) return false;  // unreachable in a DAG of lower ids

  // register bypass: in this post-order the step right before a node is its
  // last-evaluated child; when that child has no other consumer its vector
  // never needs a slot (forward D, adjoint cotangent stay in registers)
  std::vector<int> pos(ni, 0);
  for (int k = 0; k < ni; ++k) pos[order[k]] = k;
  std::vector<char> bypass(ni, 0);
  for (int r = 0; r < ni; ++r)
    bypass[r] = refs[r] == 1 && t.parent[r] >= 0 && pos[t.parent[r]] == pos[r] + 1;

  // slot simulation (bypassed vectors take no slot)
  std::vector<int> remaining(refs), slot(ni, 0xFF);
  std::set<int> free_slots;
  int top = 0, maxs = 0;
  for (int r : order) {
    for (int k = 0; k < 2; ++k) {
      const Child& cd = t.kid(r, k);
      if (cd.kind != kKindInt || bypass[cd.index]) continue;
      if (--remaining[cd.index] == 0) free_slots.insert(slot[cd.index]);
    }
    if (refs[r] > 0 && !bypass[r]) {
      int s;
      if (!free_slots.empty()) {
        s = *free_slots.begin();
        free_slots.erase(free_slots.begin());
      } else {
        s = top++;
      }
      slot[r] = s;
      maxs = std::max(maxs, s + 1);
    }
  }
  if (maxs > 250) return false;
  *n_slots = maxs;

  // deferred edges (kChildDeferred): cherries with one reached parent
  // (defer_on: defer_enabled() of this plan build)
  std::vector<char> deferred(ni, 0);
  if (defer_on)
    for (int c = 0; c < ni; ++c)
      deferred[c] = refs[c] == 1 && t.parent[c] >= 0 && t.reach[t.parent[c]] &&
                    t.kid(c, 0).kind != kKindInt && t.kid(c, 1).kind != kKindInt;

  // encode forward steps; set/accumulate flags follow the reverse order
  std::vector<char> seen(ni, 0);
  std::vector<int32_t> enc(4 * ni);
  for (int k = ni - 1; k >= 0; --k) {
    const int r = order[k];
    int32_t* e = &enc[4 * k];
    e[0] = step_row(r, slot[r]);
    for (int j = 0; j < 2; ++j) {
      const Child& cd = t.kid(r, j);
      int32_t d = child_desc(cd.kind, cd.index, cd.kind == kKindInt ? slot[cd.index] : 0);
      if (cd.kind == kKindInt) {
        if (bypass[cd.index]) d |= kChildPrev;
        if (deferred[cd.index]) d |= kChildDeferred;
        if (t.reach[r]) {
          if (seen[cd.index]) d |= kStepAccumulate;
          seen[cd.index] = 1;
        }
      }
      e[1 + j] = d;
    }
    int32_t f = 0;
    if (r == ni - 1) f |= kStepRoot;
    if (!t.reach[r]) f |= kStepUnreached;
    if (bypass[r]) f |= kStepToNext;
    if (deferred[r]) f |= kStepDeferredIn;
    e[3] = f;
  }
  if (order.back() != ni - 1) return false;
  std::memcpy(fwd, enc.data(), enc.size() * sizeof(int32_t));

  // ---- reference backtrack simulation (sankoff.py:212-265) ----
  // stack of node ids; last_parent[x] / last_slot[x] at x's LAST visit.
  const int32_t* ch = t.ch;
  std::vector<int> last_parent(ni, -1), last_slot(ni, -1);
  std::vector<char> visited(ni, 0);
  std::vector<std::pair<int, int>> stk;  // (node, parent*2+slot) ; parent -1 = root entry
  stk.push_back({t.n_all - 1, -1});
  int64_t steps = 0;
  const int64_t cap = 1LL << 22;
  bool ok = true;
  while (!stk.empty()) {
    if (++steps > cap || (int64_t)stk.size() > 4LL * t.n_all) { ok = false; break; }
    auto [node, from] = stk.back();
    stk.pop_back();
    if (node < nl) continue;  // leaves and the -1 fill are skipped
    const int x = node - nl;
    visited[x] = 1;
    if (from >= 0) { last_parent[x] = from >> 1; last_slot[x] = from & 1; }
    const int c0 = ch[2 * node], c1 = ch[2 * node + 1];
    if (c0 == node || c1 == node) { ok = false; break; }  // self loop: never terminates
    stk.push_back({c0, 2 * x + 0});
    stk.push_back({c1, 2 * x + 1});
  }
  *bt_ok = ok ? 1 : 0;
  // process order: BFS over last-parent forest from the root
  std::vector<std::vector<int>> kidsbt(ni);
  for (int x = 0; x < ni; ++x)
    if (ok && visited[x] && last_parent[x] >= 0) kidsbt[last_parent[x]].push_back(x);
  std::vector<int32_t> benc(2 * ni, 0);
  int w = 0;
  if (ok) {
    std::queue<int> q;
    q.push(ni - 1);
    std::vector<char> emitted(ni, 0);
    while (!q.empty()) {
      const int x = q.front();
      q.pop();
      if (emitted[x]) continue;
      emitted[x] = 1;
      int kind, parent = 0;
      if (x == ni - 1) {
        kind = kBtRoot;
      } else {
        parent = last_parent[x];
        const int raw = ch[2 * (nl + parent) + last_slot[x]];
        // the parent's forward used the real row only when raw < parent node
        kind = (raw < nl + parent) ? kBtReal : kBtSentinel;
      }
      benc[2 * w] = (x & 0xFFFF) | (kind << 16) | (last_slot[x] > 0 ? (1 << 20) : 0);
      benc[2 * w + 1] = parent;
      ++w;
      for (int c : kidsbt[x]) q.push(c);
    }
    for (int x = 0; x < ni; ++x) {
      if (!emitted[x]) {
        benc[2 * w] = (x & 0xFFFF) | (kBtUnreached << 16);
        benc[2 * w + 1] = 0;
        ++w;
      }
    }
  }
  std::memcpy(bt, benc.data(), benc.size() * sizeof(int32_t));
  return true;
}

// Staged program of one tree (layout: trex_common.h).  Nodes are levelled by
// height over real internal edges (a leaf / 1e5-row child adds nothing), each
// level is one stage, its nodes dealt round-robin to the workgroup's waves:
// a stage's nodes depend only on earlier stages, so the waves run them in
// parallel and the serial chain is the tree height (6 for a balanced
// 64-taxon tree instead of 63 nodes).  A topology with a shared internal
// child (trex's DAG quirk) runs serially on wave 0 in index order, where the
// accumulate flags order its cotangent sums exactly as the single-wave
// kernels do.
void stage_one_tree(const TreeShape& t, int32_t* region) {
  const int ni = t.ni;
  constexpr int W = kStageWaves;
  // (stage, wave) of every row
  int S = 1;
  std::vector<int> stage(ni, 0), wave(ni, 0);
  if (!t.n_dag) {
    S = *std::max_element(t.height.begin(), t.height.end());
    std::vector<int> fill(S, 0);
    for (int r = 0; r < ni; ++r) {
      stage[r] = t.height[r] - 1;
      wave[r] = fill[stage[r]]++ % W;
    }
  }
  std::vector<int> order(ni);
  for (int r = 0; r < ni; ++r) order[r] = r;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
    return stage[x] != stage[y] ? stage[x] < stage[y] : wave[x] < wave[y];
  });
  int32_t* steps = region;
  region[4LL * ni] = S;
  bucket_offsets(region + 4LL * ni + 1, S * W, ni,
                 [&](int k) { return stage[order[k]] * W + wave[order[k]]; });
  // accumulate flags follow the adjoint's order: stages, then steps, reversed
  std::vector<char> seen(ni, 0);
  for (int k = ni - 1; k >= 0; --k) {
    const int r = order[k];
    int32_t* e = steps + 4LL * k;
    e[0] = step_row(r);
    for (int j = 0; j < 2; ++j) {
      const Child& cd = t.kid(r, j);
      int32_t d = child_desc(cd.kind, cd.index);
      if (cd.kind == kKindInt && t.reach[r]) {
        if (seen[cd.index]) d |= kStepAccumulate;
        seen[cd.index] = 1;
      }
      e[1 + j] = d;
    }
    e[3] = (r == ni - 1 ? kStepRoot : 0) | (t.reach[r] ? 0 : kStepUnreached);
  }
}

// Lane-per-site program of one tree (layout: trex_common.h).  Internal rows
// of height <= 2 are computed inline by the task that consumes them; every
// other row (and the root) is a task.  A task's stage is its height - 3 (the
// root's at least 0), so a stage depends only on earlier stages.  A task
// row's LDS slot holds its D from its own stage to its parent's (the root's:
// its own stage), then, in the reversed adjoint, its cotangent over the same
// interval: slots are
// interval-coloured, reused once the interval has ended.  Returns the slot
// count, or -1 when the tree cannot run this program (a shared internal
// child -- trex's DAG quirk --, an internal row the root does not reach, or
// more than 255 slots); the other kernels then serve the batch.
int lane_program_one_tree(const TreeShape& t, int32_t* region) {
  const int ni = t.ni;
  std::memset(region, 0, sizeof(int32_t) * lp_tree_ints(ni));
  region[1] = -1;
  if (t.n_dag || t.n_unreached) return -1;
  const int root = ni - 1;
  std::vector<char> task(ni, 0);
  std::vector<int> stage(ni, 0);
  int S = 1;
  for (int r = 0; r < ni; ++r) {
    task[r] = r == root || t.height[r] >= 3;
    stage[r] = std::max(0, t.height[r] - 3);
    if (task[r]) S = std::max(S, stage[r] + 1);
  }
  // slots: interval colouring over [stage(r), stage(parent(r))]
  std::vector<int> order;
  for (int r = 0; r < ni; ++r)
    if (task[r]) order.push_back(r);
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return stage[x] < stage[y]; });
  std::vector<int> slot(ni, 0xFF), slot_end;
  for (int r : order) {
    const int st = stage[r], en = r == root ? stage[r] : stage[t.parent[r]];
    int s = 0;
    while (s < (int)slot_end.size() && slot_end[s] >= st) ++s;
    if (s == (int)slot_end.size()) slot_end.push_back(en);
    else slot_end[s] = en;
    slot[r] = s;
  }
  const int n_slots = (int)slot_end.size();
  if (n_slots > 255) return -1;
  // inline rows in post-order of their task (children first): index list
  std::vector<int> inl(ni, -1);
  std::vector<int32_t> ient;
  std::function<int32_t(int, int)> desc = [&](int r, int k) -> int32_t {
    const Child& cd = t.kid(r, k);
    const int c = cd.index;
    if (cd.kind != kKindInt) return child_desc(cd.kind, c);
    if (task[c]) return child_desc(kKindInt, c, slot[c]);
    const int32_t d0 = desc(c, 0), d1 = desc(c, 1);
    inl[c] = (int)(ient.size() / 4);
    ient.insert(ient.end(), {c, d0, d1, t.height[c]});
    return child_desc(kKindInline, inl[c]);
  };
  const int n_steps = (int)order.size();
  int32_t* steps = region + lp_steps_offset(ni);
  bucket_offsets(region + 4, S, n_steps, [&](int k) { return stage[order[k]]; });
  for (int k = 0; k < n_steps; ++k) {
    const int r = order[k];
    steps[4 * k] = step_row(r, slot[r]);
    steps[4 * k + 1] = desc(r, 0);
    steps[4 * k + 2] = desc(r, 1);
    steps[4 * k + 3] = r == root ? kStepRoot : 0;
  }
  if (!ient.empty()) std::memcpy(steps + 4LL * n_steps, ient.data(), ient.size() * sizeof(int32_t));
  region[0] = S;
  region[1] = n_slots;
  region[2] = n_steps;
  region[3] = (int)(ient.size() / 4);
  return n_slots;
}

}  // namespace

}  // namespace trex

extern "C" int64_t trex_plan_ints(int B, int n_all) {
  if (B <= 0 || n_all < 2) return 0;
  return trex::plan_layout(B, trex::tree_ni(n_all)).total;
}

extern "C" int trex_plan_build(const int32_t* children, int B, int n_all,
                               int32_t* plan, int32_t* info) {
  using namespace trex;
  if (!children || !plan || !uniform_shape(B, n_all))
    return set_error(TREX_E_ARG, "trex_plan_build: bad arguments (B=%d n_all=%d)", B, n_all);
  const int nl = tree_nl(n_all), ni = n_all - nl;
  const PlanLayout lay = plan_layout(B, ni);
  plan[0] = 0;  // not a plan until its header is written
  int max_slots = 0, all_bt_ok = 1, dag = 0, unr = 0, lp_slots = 0;
  const bool defer_on = defer_enabled();
  TreeShape t;
  for (int b = 0; b < B; ++b) {
    int s = 0, ok = 0;
    if (!analyse_tree(children + (int64_t)b * n_all * 2, n_all, t) ||
        !plan_one_tree(t, defer_on, plan + lay.fwd + (int64_t)b * ni * 4,
                       plan + lay.bt + (int64_t)b * ni * 2, &s, &ok))
      return set_error(TREX_E_TOPOLOGY, "trex_plan_build: tree %d has an invalid child list", b);
    stage_one_tree(t, plan + lay.staged + b * staged_tree_ints(ni));
    const int ls = lane_program_one_tree(t, plan + lay.lanes + b * lp_tree_ints(ni));
    lp_slots = (ls < 0 || lp_slots < 0) ? -1 : std::max(lp_slots, ls);
    max_slots = std::max(max_slots, s);
    all_bt_ok &= ok;
    dag += t.n_dag;
    unr += t.n_unreached;
  }
  write_header(plan, kPlanMagic, {B, n_all, nl, ni, max_slots, all_bt_ok, lp_slots});
  if (info) {
    // low 16 bits: the stack depth; bits 16-23: lane-program slots + 1 (0: a
    // tree of the batch cannot run the lane-per-site kernel)
    info[0] = max_slots | ((lp_slots < 0 ? 0 : lp_slots + 1) << 16);
    info[1] = all_bt_ok;
    info[2] = dag;
    info[3] = unr;
  }
  return TREX_OK;
}

// ---------------------------------------------------------------------------
// Fused Q = 4 program: the forward steps of a built plan, one decoded record
// per step (layout: trex_common.h).  The plan is read, never written; the
// deferral bits are the plan's own (the TREX_DEFER state it was built with).
// Refused with TREX_E_UNSUPPORTED (the caller keeps the generic kernel): a
// 1e5-sentinel child, a step the root does not reach, a node with two parents.
// ---------------------------------------------------------------------------
extern "C" int64_t trex_fused4_program_ints(int B, int n_all) {
  if (!trex::uniform_shape(B, n_all)) return 0;
  return TREX_PLAN_HEADER_INTS + (int64_t)B * trex::tree_ni(n_all) * trex::kF4RecInts;
}

extern "C" int trex_fused4_program_build(const int32_t* plan, int B, int n_all, int32_t* prog) {
  using namespace trex;
  const char* fn = "trex_fused4_program_build";
  if (!plan || !prog || !uniform_shape(B, n_all))
    return set_error(TREX_E_ARG, "%s: bad arguments (B=%d n_all=%d)", fn, B, n_all);
  if (plan[0] != kPlanMagic || plan[1] != B || plan[2] != n_all)
    return set_error(TREX_E_ARG, "%s: not a plan of trex_plan_build for B=%d n_all=%d", fn, B,
                     n_all);
  const int ni = tree_ni(n_all);
  const int32_t* fwd = plan + plan_layout(B, ni).fwd;
  prog[0] = 0;  // not a program until its header is written
  int32_t* rec = prog + TREX_PLAN_HEADER_INTS;
  constexpr int kSlotBytes = 4 * 64 * 4;  // [64 lanes][Q = 4] f32
  constexpr int kLeafRowBytes = 64;       // [64 lanes] i8
  for (int64_t t = 0; t < (int64_t)B * ni; ++t) {
    const int32_t* e = fwd + 4 * t;
    int32_t* r = rec + kF4RecInts * t;
    const int tree = (int)(t / ni);
    if (e[3] & kStepUnreached)
      return set_error(TREX_E_UNSUPPORTED, "%s: tree %d has a row the root does not reach", fn,
                       tree);
    int32_t flags = 0;
    bool leaf[2];
    for (int c = 0; c < 2; ++c) {
      const int32_t d = e[1 + c];
      const int kind = desc_kind(d);
      if (kind != kKindLeaf && kind != kKindInt)
        return set_error(TREX_E_UNSUPPORTED, "%s: tree %d has a 1e5-sentinel child", fn, tree);
      if (d & kStepAccumulate)
        return set_error(TREX_E_UNSUPPORTED, "%s: tree %d has a node with two parents", fn, tree);
      leaf[c] = kind == kKindLeaf;
      r[5 + c] = kF4NoRow;
      if (leaf[c]) {
        flags |= c == 0 ? kF4Leaf0 : kF4Leaf1;
        r[2 + c] = desc_index(d) * kLeafRowBytes;
      } else {
        const bool prev = (d & kChildPrev) != 0, deferred = (d & kChildDeferred) != 0;
        if (prev) flags |= c == 0 ? kF4Prev0 : kF4Prev1;
        if (deferred) flags |= c == 0 ? kF4Defer0 : kF4Defer1;
        r[2 + c] = prev ? 0 : desc_slot(d) * kSlotBytes;
        if (!deferred) r[5 + c] = desc_index(d);
      }
    }
    const bool cherry = leaf[0] && leaf[1];
    if ((e[3] & kStepDeferredIn) && !cherry)
      return set_error(TREX_E_ARG, "%s: tree %d: a deferred step that is no cherry", fn, tree);
    const int oslot = desc_slot(e[0]);
    if (e[3] & kStepDeferredIn) flags |= kF4DeferIn;
    if (e[3] & kStepToNext) flags |= kF4ToNext;
    if (e[3] & kStepRoot) flags |= kF4Root;
    const bool put = !(e[3] & kStepToNext) && oslot != 0xFF;
    if (put) flags |= kF4Put;
    const int fcls = cherry ? ((e[3] & kStepDeferredIn) ? kF4CherryDeferred : kF4Cherry)
                     : (leaf[0] || leaf[1]) ? kF4LeafInt : kF4IntInt;
    r[0] = flags | (fcls << kF4FwdClassShift);
    r[1] = desc_index(e[0]);
    r[4] = put ? oslot * kSlotBytes : 0;
    r[7] = 0;
  }
  write_header(prog, kF4Magic, {B, n_all, ni});
  return TREX_OK;
}

// ---------------------------------------------------------------------------
// Ragged batches: trees of different sizes (n_all_b) and site counts (L_b) in
// one launch (layout and per-tree record: trex_common.h, ragged_layout).
// ---------------------------------------------------------------------------
namespace trex {
namespace {
bool ragged_shapes(const int32_t* n_all, const int32_t* L, int B, int64_t* steps, int64_t* items) {
  *steps = 0;
  *items = 0;
  for (int b = 0; b < B; ++b) {
    if (!uniform_shape(1, n_all[b]) || L[b] <= 0) return false;
    *steps += tree_ni(n_all[b]);
    *items += (L[b] + 63) / 64;
  }
  return *items <= 0x7FFFFFFF;
}
}  // namespace
}  // namespace trex

extern "C" int64_t trex_ragged_plan_ints(int B, const int32_t* n_all, const int32_t* L) {
  if (B <= 0 || !n_all || !L) return 0;
  int64_t steps, items;
  if (!trex::ragged_shapes(n_all, L, B, &steps, &items)) return 0;
  return trex::ragged_layout(B, items, steps).total;
}

extern "C" int trex_ragged_plan_build(const int32_t* children, const int32_t* n_all,
                                      const int32_t* L, int B, int32_t* plan, int64_t* info) {
  using namespace trex;
  int64_t steps, items;
  if (!children || !n_all || !L || !plan || B <= 0 || !ragged_shapes(n_all, L, B, &steps, &items))
    return set_error(TREX_E_ARG, "trex_ragged_plan_build: bad arguments (B=%d)", B);
  const RaggedLayout lay = ragged_layout(B, items, steps);
  int32_t* ritem = plan + lay.item;
  plan[0] = 0;  // not a plan until its header is written
  int64_t step_off = 0, item_off = 0, site_off = 0, leaf_off = 0, rows_off = 0, child_off = 0;
  int max_slots = 0, max_nl = 0, max_ni = 0, all_ok = 1, dag = 0, unr = 0;
  const bool defer_on = defer_enabled();
  TreeShape t;
  for (int b = 0; b < B; ++b) {
    int s = 0, ok = 0;
    if (!analyse_tree(children + child_off, n_all[b], t) ||
        !plan_one_tree(t, defer_on, plan + lay.fwd + step_off * 4, plan + lay.bt + step_off * 2,
                       &s, &ok))
      return set_error(TREX_E_TOPOLOGY, "trex_ragged_plan_build: tree %d has an invalid child list",
                       b);
    const int nl = t.nl, ni = t.ni;
    if (site_off > 0x7FFFFFFF)
      return set_error(TREX_E_UNSUPPORTED, "trex_ragged_plan_build: more than 2^31 sites");
    if ((int64_t)ni * L[b] * 4 * 4 > 0x7FFFFFF0LL)
      return set_error(TREX_E_UNSUPPORTED, "trex_ragged_plan_build: tree %d's DP table exceeds 2 GiB",
                       b);
    int32_t* m = plan + lay.meta + (int64_t)b * kRaggedMeta;
    m[kRecStep] = (int32_t)step_off;
    m[kRecNInt] = ni;
    m[kRecNLeaves] = nl;
    m[kRecL] = L[b];
    m[kRecSite] = (int32_t)site_off;
    m[kRecItem] = (int32_t)item_off;
    m[kRecLeafLo] = (int32_t)(leaf_off & 0xFFFFFFFF);
    m[kRecLeafHi] = (int32_t)(leaf_off >> 32);
    m[kRecRowsLo] = (int32_t)(rows_off & 0xFFFFFFFF);
    m[kRecRowsHi] = (int32_t)(rows_off >> 32);
    const int tiles = (L[b] + 63) / 64;
    for (int i = 0; i < tiles; ++i) ritem[item_off + i] = b;
    max_slots = std::max(max_slots, s);
    max_nl = std::max(max_nl, nl);
    max_ni = std::max(max_ni, ni);
    all_ok &= ok;
    dag += t.n_dag;
    unr += t.n_unreached;
    step_off += ni;
    item_off += tiles;
    site_off += L[b];
    leaf_off += (int64_t)nl * L[b];
    rows_off += (int64_t)ni * L[b];
    child_off += 2LL * n_all[b];
  }
  write_header(plan, kRaggedMagic,
               {B, (int32_t)steps, (int32_t)items, max_slots, max_nl, all_ok, max_ni});
  if (info) {
    info[0] = max_slots;  // n_slots for the launch
    info[1] = max_nl;     // LDS leaf tile rows
    info[2] = items;      // work items (64-site tiles)
    info[3] = leaf_off;   // packed leaf bytes: sum n_leaves_b * L_b
    info[4] = rows_off;   // packed DP row-sites: sum n_int_b * L_b (x Q floats)
    info[5] = site_off;   // packed sites: sum L_b
    info[6] = all_ok;     // reference backtrack terminates on every tree
    info[7] = dag + ((int64_t)unr << 32);
  }
  return TREX_OK;
}

// ---------------------------------------------------------------------------
// NNI plan (sankoff_rows.h): the pre-order "outside" pass and the per-edge
// neighbour scores.  Layout (ints): header [16] | per tree a region of
// nni_tree_ints(ni) ints: pre-order entries [ni][4] | move entries
// [ni - 1][4].
//   pre-order entry: {internal row, parent row (-1: the root), sibling
//     descriptor, 0}; a DFS from the root, so a node's parent comes before it
//   move entry e (v = n_leaves + e, never the root): {u row, a0 descriptor,
//     a1 descriptor, s descriptor}: u = v's parent, (a0, a1) = children[v] in
//     stored order, s = v's sibling
//   descriptor: node_desc (trex_common.h), kind << 24 | index (kind 1: leaf
//     index, 2: internal row)
// Attach plan (sankoff_rows.h, attach_score_kernel; sankoff_sets.hip,
// sets_fwd_kernel walks it as a post-order): the edges of every tree
// grouped by their upper node.  Layout (ints): header [16] | per tree
// [ni][4]: entry r = {internal row r, descriptor of child 0, descriptor of
// child 1, 1 if r is the root else 0}, rows ascending, children in stored
// order, descriptors as in the NNI plan.
// Only proper rooted binary trees have neighbours or attachment edges:
// everything trex's child rule tolerates beyond them (-1 fills, forward
// references, shared or orphan rows) is refused by both with TREX_E_TOPOLOGY.
// ---------------------------------------------------------------------------
namespace trex {
namespace {
inline int64_t nni_tree_ints(int ni) { return 8LL * ni - 4; }
inline int64_t attach_tree_ints(int ni) { return 4LL * ni; }

// nullptr when the tree is a proper rooted binary tree (parent[] is then
// filled), else what is wrong
const char* proper_tree_parents(const int32_t* ch, int n_all, std::vector<int>& parent) {
  const int nl = tree_nl(n_all);
  parent.assign(n_all, -1);
  for (int node = nl; node < n_all; ++node) {
    const int c0 = ch[2 * node], c1 = ch[2 * node + 1];
    if (c0 < 0 || c1 < 0) return "a child is missing (-1 fill)";
    if (c0 >= node || c1 >= node) return "a child id is not below its parent's";
    if (c0 == c1) return "a node lists the same child twice";
    if (parent[c0] >= 0 || parent[c1] >= 0) return "a node has two parents";
    parent[c0] = node;
    parent[c1] = node;
  }
  // 2 ni child slots, all distinct, over the n_all - 1 = 2 ni nodes below the
  // root: every one of them has exactly one parent, of a higher id, so every
  // path leads up to the root n_all - 1
  return nullptr;
}

const char* nni_one_tree(const int32_t* ch, int n_all, int32_t* region) {
  const int nl = tree_nl(n_all), ni = n_all - nl;
  std::vector<int> parent;
  if (const char* why = proper_tree_parents(ch, n_all, parent)) return why;
  auto sibling = [&](int c) {
    const int p = parent[c];
    return ch[2 * p] == c ? ch[2 * p + 1] : ch[2 * p];
  };
  int32_t* pre = region;
  int32_t* mv = region + 4LL * ni;
  std::vector<int> st;
  st.push_back(n_all - 1);
  int w = 0;
  while (!st.empty()) {
    const int node = st.back();
    st.pop_back();
    pre[4 * w] = node - nl;
    pre[4 * w + 1] = node == n_all - 1 ? -1 : parent[node] - nl;
    pre[4 * w + 2] = node == n_all - 1 ? 0 : node_desc(sibling(node), nl);
    pre[4 * w + 3] = 0;
    ++w;
    for (int k = 1; k >= 0; --k)
      if (ch[2 * node + k] >= nl) st.push_back(ch[2 * node + k]);
  }
  if (w != ni) return "an internal node is not reachable from the root";
  for (int e = 0; e < ni - 1; ++e) {
    const int v = nl + e;
    mv[4 * e] = parent[v] - nl;
    mv[4 * e + 1] = node_desc(ch[2 * v], nl);
    mv[4 * e + 2] = node_desc(ch[2 * v + 1], nl);
    mv[4 * e + 3] = node_desc(sibling(v), nl);
  }
  return nullptr;
}

const char* attach_one_tree(const int32_t* ch, int n_all, int32_t* region) {
  const int nl = tree_nl(n_all), ni = n_all - nl;
  std::vector<int> parent;
  if (const char* why = proper_tree_parents(ch, n_all, parent)) return why;
  for (int r = 0; r < ni; ++r) {
    region[4 * r] = r;
    for (int k = 0; k < 2; ++k) region[4 * r + 1 + k] = node_desc(ch[2 * (nl + r) + k], nl);
    region[4 * r + 3] = r == ni - 1 ? 1 : 0;
  }
  return nullptr;
}

// SPR plan (sankoff_spr.hip; layout: include/trex_hip.h): per node its parent,
// sibling and the entry / exit numbers of a pre-order DFS over all nodes
// (children in stored order), then the internal nodes by ascending entry with
// their children's ids
const char* spr_one_tree(const int32_t* ch, int n_all, int32_t* region) {
  const int nl = tree_nl(n_all), ni = n_all - nl;
  std::vector<int> parent;
  if (const char* why = proper_tree_parents(ch, n_all, parent)) return why;
  int32_t* node = region;
  int32_t* walk = region + 4LL * n_all;
  std::vector<int> st;
  st.push_back(n_all - 1);
  int entry = 0, w = 0;
  while (!st.empty()) {
    const int x = st.back();
    st.pop_back();
    const int p = parent[x];
    node[4 * x] = p;
    node[4 * x + 1] = p < 0 ? -1 : (ch[2 * p] == x ? ch[2 * p + 1] : ch[2 * p]);
    node[4 * x + 2] = entry++;
    if (x < nl) continue;
    walk[4 * w] = x - nl;
    walk[4 * w + 1] = ch[2 * x];
    walk[4 * w + 2] = ch[2 * x + 1];
    walk[4 * w + 3] = 0;
    ++w;
    st.push_back(ch[2 * x + 1]);
    st.push_back(ch[2 * x]);
  }
  if (w != ni || entry != n_all) return "a node is not reachable from the root";
  // subtree sizes: children have lower ids than their parents
  std::vector<int> size(n_all, 1);
  for (int x = nl; x < n_all; ++x) size[x] += size[ch[2 * x]] + size[ch[2 * x + 1]];
  for (int x = 0; x < n_all; ++x) node[4 * x + 3] = node[4 * x + 2] + size[x];
  return nullptr;
}

// the builders: header | one region of tree_ints per tree, written by one_tree
int proper_plan_build(const char* fn, const char* two_leaves, int32_t magic,
                      const int32_t* children, int B, int n_all, int32_t* plan,
                      int64_t (*tree_ints_of)(int),
                      const char* (*one_tree)(const int32_t*, int, int32_t*)) {
  if (!children || !plan || !uniform_shape(B, n_all) || n_all % 2 == 0)
    return set_error(TREX_E_ARG, "%s: bad arguments (B=%d n_all=%d)", fn, B, n_all);
  const int nl = tree_nl(n_all);
  const int64_t tree_ints = tree_ints_of(n_all - nl);
  if (nl < 3)
    return set_error(TREX_E_TOPOLOGY, "%s: a tree of %d leaves %s (3 or more are needed)", fn, nl,
                     two_leaves);
  plan[0] = 0;  // not a plan until its header is written
  for (int b = 0; b < B; ++b)
    if (const char* why = one_tree(children + (int64_t)b * n_all * 2, n_all,
                                   plan + TREX_PLAN_HEADER_INTS + b * tree_ints))
      return set_error(TREX_E_TOPOLOGY, "%s: tree %d is not a proper rooted binary tree: %s", fn,
                       b, why);
  write_header(plan, magic, {B, n_all, nl, n_all - nl});
  return TREX_OK;
}
}  // namespace
}  // namespace trex

extern "C" int64_t trex_nni_plan_ints(int B, int n_all) {
  if (!trex::uniform_shape(B, n_all)) return 0;
  return TREX_PLAN_HEADER_INTS + B * trex::nni_tree_ints(trex::tree_ni(n_all));
}

extern "C" int trex_nni_plan_build(const int32_t* children, int B, int n_all, int32_t* nni_plan) {
  using namespace trex;
  return proper_plan_build("trex_nni_plan_build", "has no NNI neighbours", kNniMagic, children, B,
                           n_all, nni_plan, nni_tree_ints, nni_one_tree);
}

extern "C" int64_t trex_attach_plan_ints(int B, int n_all) {
  if (!trex::uniform_shape(B, n_all)) return 0;
  return TREX_PLAN_HEADER_INTS + B * trex::attach_tree_ints(trex::tree_ni(n_all));
}

extern "C" int trex_attach_plan_build(const int32_t* children, int B, int n_all,
                                      int32_t* attach_plan) {
  using namespace trex;
  return proper_plan_build("trex_attach_plan_build", "is not supported", kAttachMagic, children, B,
                           n_all, attach_plan, attach_tree_ints, attach_one_tree);
}

extern "C" int64_t trex_spr_plan_ints(int B, int n_all) {
  if (!trex::uniform_shape(B, n_all)) return 0;
  return TREX_PLAN_HEADER_INTS + B * trex::spr_tree_ints(trex::tree_ni(n_all));
}

extern "C" int trex_spr_plan_build(const int32_t* children, int B, int n_all, int32_t* spr_plan) {
  using namespace trex;
  return proper_plan_build("trex_spr_plan_build", "has no SPR neighbours", kSprMagic, children, B,
                           n_all, spr_plan, spr_tree_ints, spr_one_tree);
}
