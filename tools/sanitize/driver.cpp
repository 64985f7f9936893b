// AddressSanitizer / UBSan driver for the host-side code the GPU path and
// its checker depend on (SURVEY.md §5 "sanitizers"):
//   * trex_amd/csrc/plan.cpp -- the topology planner (uniform and ragged
//     batches) on random, quirky (-1 fills, forward references, DAGs,
//     orphans), cyclic and malformed child lists, writing into buffers sized
//     exactly by trex_plan_ints / trex_ragged_plan_ints, the fused Q = 4
//     program (trex_fused4_program_build) of every accepted uniform plan, its
//     accepted records range-checked, and the NNI planner
//     (trex_nni_plan_build), the attach planner (trex_attach_plan_build) and
//     the SPR planner (trex_spr_plan_build) on the same trees, their accepted
//     plans range-checked;
//   * oracle/cpu_port.c -- the OpenMP C restatement (the CPU baseline and a
//     test checker) on random trees, Q = 2..20, hard and softmin, with and
//     without the DP table output.
// Built by tools/sanitize/Makefile with -fsanitize=address,undefined
// -fno-sanitize-recover=all; any report aborts with a non-zero exit.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../include/trex_hip.h"

namespace trex {
// plan.cpp reports errors through the library's set_error (sankoff.hip)
int set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  char buf[512];
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace trex

extern "C" int sankoff_cpu_fwd_bwd(const int32_t* children, const int8_t* leaves,
                                   const float* cost, int B, int L, int n_all, int Q, float tau,
                                   float* dp_out, double* tree_score, double* d_cost,
                                   int want_grad, int nthreads);

namespace {

std::mt19937 rng(12345);

int rnd(int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); }

// coalescent merge: child ids below the parent (trex's numbering)
void random_tree(int nl, int32_t* ch) {
  const int n_all = 2 * nl - 1;
  for (int i = 0; i < 2 * n_all; ++i) ch[i] = -1;
  std::vector<int> active;
  for (int i = 0; i < nl; ++i) active.push_back(i);
  for (int k = 0; k < nl - 1; ++k) {
    const int a = rnd(0, (int)active.size() - 1);
    int b = rnd(0, (int)active.size() - 2);
    if (b >= a) ++b;
    const int ca = active[a], cb = active[b];
    const int parent = nl + k;
    ch[2 * parent] = std::min(ca, cb);
    ch[2 * parent + 1] = std::max(ca, cb);
    active.erase(active.begin() + std::max(a, b));
    active.erase(active.begin() + std::min(a, b));
    active.push_back(parent);
  }
}

// the quirks trex's child rule allows (sankoff.py:60,67)
void perturb(int nl, int32_t* ch, int mode) {
  const int n_all = 2 * nl - 1;
  const int node = rnd(nl, n_all - 1);
  switch (mode) {
    case 0: ch[2 * node + 1] = -1; break;                       // -1 fill
    case 1: ch[2 * node] = rnd(node, n_all - 1); break;         // forward ref / self
    case 2: ch[2 * node] = rnd(nl, std::max(nl, node - 1)); break;  // DAG / orphan
    case 3: ch[2 * node] = n_all + 3; break;                    // malformed (rejected)
    default: break;
  }
}

// the fused Q = 4 program of an accepted plan, into a buffer of exactly
// trex_fused4_program_ints; an accepted program's records stay in range: rows
// below ni, operand offsets inside the leaf tile / the slot stack
int check_fused4(const std::vector<int32_t>& plan, int B, int n_all, int n_slots, int* built) {
  const int nl = (n_all + 1) / 2, ni = n_all - nl;
  const int64_t n = trex_fused4_program_ints(B, n_all);
  if (n != TREX_PLAN_HEADER_INTS + (int64_t)B * ni * 8) return 20;
  std::vector<int32_t> prog((size_t)n);
  const int rc = trex_fused4_program_build(plan.data(), B, n_all, prog.data());
  if (rc == TREX_E_UNSUPPORTED) return 0;  // a quirky tree: the generic kernel's
  if (rc != 0) return 21;
  ++*built;
  for (int64_t t = 0; t < (int64_t)B * ni; ++t) {
    const int32_t* r = prog.data() + TREX_PLAN_HEADER_INTS + 8 * t;
    const bool leaf[2] = {(r[0] & 1) != 0, (r[0] & 2) != 0};  // kF4Leaf0 / kF4Leaf1
    if (r[1] < 0 || r[1] >= ni) return 22;
    for (int c = 0; c < 2; ++c) {
      const int32_t lim = leaf[c] ? nl * 64 : n_slots * 1024;  // 0: kF4Prev* (bypass)
      if (r[2 + c] < 0 || (r[2 + c] >= lim && r[2 + c] != 0)) return 23;
      if (r[5 + c] != -1 && (leaf[c] || r[5 + c] < 0 || r[5 + c] >= ni)) return 24;
    }
    if (r[4] < 0 || (r[4] >= n_slots * 1024 && r[4] != 0)) return 25;
  }
  return 0;
}

int check_uniform() {
  int runs = 0, fused = 0;
  for (int it = 0; it < 400; ++it) {
    const int nl = rnd(2, 128);
    const int n_all = 2 * nl - 1;
    const int B = rnd(1, 6);
    std::vector<int32_t> ch((size_t)B * n_all * 2);
    for (int b = 0; b < B; ++b) {
      random_tree(nl, ch.data() + (size_t)b * n_all * 2);
      if (it % 2) perturb(nl, ch.data() + (size_t)b * n_all * 2, rnd(0, 4));
    }
    const int64_t n = trex_plan_ints(B, n_all);
    if (n <= 0) continue;  // n_all < 3 is rejected by trex_plan_ints / trex_plan_build
    std::vector<int32_t> plan((size_t)n);
    int32_t info[4];
    const int rc = trex_plan_build(ch.data(), B, n_all, plan.data(), info);
    if (rc != 0 && rc != TREX_E_TOPOLOGY && rc != TREX_E_ARG) return 1;
    if (rc == 0)
      if (int e = check_fused4(plan, B, n_all, info[0] & 0xFFFF, &fused)) return e;
    ++runs;
  }
  std::printf("uniform plans: %d, fused Q = 4 programs: %d\n", runs, fused);
  return 0;
}

// the NNI planner accepts proper binary trees only: every perturbed tree is
// either refused or still proper, and an accepted plan's words stay in range
int check_nni() {
  int built = 0, refused = 0;
  for (int it = 0; it < 400; ++it) {
    const int nl = rnd(2, 128);
    const int n_all = 2 * nl - 1;
    const int ni = n_all - nl;
    const int B = rnd(1, 6);
    std::vector<int32_t> ch((size_t)B * n_all * 2);
    bool clean = true;
    for (int b = 0; b < B; ++b) {
      random_tree(nl, ch.data() + (size_t)b * n_all * 2);
      if (it % 2) {
        const int mode = rnd(0, 4);
        perturb(nl, ch.data() + (size_t)b * n_all * 2, mode);
        clean = clean && mode == 4;
      }
    }
    const int64_t n = trex_nni_plan_ints(B, n_all);
    if (n <= 0) return 5;
    std::vector<int32_t> plan((size_t)n);
    const int rc = trex_nni_plan_build(ch.data(), B, n_all, plan.data());
    if (rc != 0 && rc != TREX_E_TOPOLOGY && rc != TREX_E_ARG) return 6;
    if (clean && nl >= 3 && rc != 0) return 7;  // a coalescent tree is proper
    if (nl < 3 && rc == 0) return 8;
    if (rc != 0) {
      ++refused;
      continue;
    }
    ++built;
    for (int b = 0; b < B; ++b) {
      const int32_t* r = plan.data() + TREX_PLAN_HEADER_INTS + (size_t)b * (8 * ni - 4);
      auto desc_ok = [&](int32_t d) {
        const int kind = d >> 24, idx = d & 0xFFFF;
        return (kind == 1 && idx < nl) || (kind == 2 && idx < ni);
      };
      if (r[0] != ni - 1 || r[1] != -1) return 9;  // pre-order starts at the root
      for (int k = 1; k < ni; ++k)
        if (r[4 * k] < 0 || r[4 * k] >= ni || r[4 * k + 1] <= r[4 * k] || r[4 * k + 1] >= ni ||
            !desc_ok(r[4 * k + 2]))
          return 10;
      const int32_t* mv = r + 4 * ni;
      for (int e = 0; e < ni - 1; ++e)
        if (mv[4 * e] <= e || mv[4 * e] >= ni || !desc_ok(mv[4 * e + 1]) ||
            !desc_ok(mv[4 * e + 2]) || !desc_ok(mv[4 * e + 3]))
          return 11;
    }
  }
  std::printf("nni plans: %d built, %d refused\n", built, refused);
  return 0;
}

// the attach planner accepts the same trees as the NNI planner; an accepted
// plan lists every node below the root once, as a child of an ascending row
int check_attach() {
  int built = 0, refused = 0;
  for (int it = 0; it < 400; ++it) {
    const int nl = rnd(2, 128);
    const int n_all = 2 * nl - 1;
    const int ni = n_all - nl;
    const int B = rnd(1, 6);
    std::vector<int32_t> ch((size_t)B * n_all * 2);
    bool clean = true;
    for (int b = 0; b < B; ++b) {
      random_tree(nl, ch.data() + (size_t)b * n_all * 2);
      if (it % 2) {
        const int mode = rnd(0, 4);
        perturb(nl, ch.data() + (size_t)b * n_all * 2, mode);
        clean = clean && mode == 4;
      }
    }
    const int64_t n = trex_attach_plan_ints(B, n_all);
    if (n != TREX_PLAN_HEADER_INTS + (int64_t)B * ni * 4) return 12;
    std::vector<int32_t> plan((size_t)n), nni((size_t)trex_nni_plan_ints(B, n_all));
    const int rc = trex_attach_plan_build(ch.data(), B, n_all, plan.data());
    if (rc != 0 && rc != TREX_E_TOPOLOGY && rc != TREX_E_ARG) return 13;
    if (rc != trex_nni_plan_build(ch.data(), B, n_all, nni.data())) return 14;  // same rule
    if (clean && nl >= 3 && rc != 0) return 15;
    if (nl < 3 && rc == 0) return 16;
    if (rc != 0) {
      ++refused;
      continue;
    }
    ++built;
    for (int b = 0; b < B; ++b) {
      const int32_t* r = plan.data() + TREX_PLAN_HEADER_INTS + (size_t)b * ni * 4;
      std::vector<int> seen(n_all, 0);
      for (int k = 0; k < ni; ++k) {
        if (r[4 * k] != k || r[4 * k + 3] != (k == ni - 1 ? 1 : 0)) return 17;
        for (int c = 1; c <= 2; ++c) {
          const int kind = r[4 * k + c] >> 24, idx = r[4 * k + c] & 0xFFFF;
          if (!((kind == 1 && idx < nl) || (kind == 2 && idx < k))) return 18;
          ++seen[kind == 1 ? idx : nl + idx];
        }
      }
      for (int x = 0; x < n_all - 1; ++x)
        if (seen[x] != 1) return 19;
    }
  }
  std::printf("attach plans: %d built, %d refused\n", built, refused);
  return 0;
}

// the SPR planner accepts the same trees as the NNI planner; an accepted
// plan's node records nest like the tree (a node's interval inside its
// parent's, siblings' intervals adjacent) and its walk lists every internal
// row once, a parent before its children
int check_spr() {
  int built = 0, refused = 0;
  for (int it = 0; it < 400; ++it) {
    const int nl = rnd(2, 128);
    const int n_all = 2 * nl - 1;
    const int ni = n_all - nl;
    const int B = rnd(1, 6);
    std::vector<int32_t> ch((size_t)B * n_all * 2);
    bool clean = true;
    for (int b = 0; b < B; ++b) {
      random_tree(nl, ch.data() + (size_t)b * n_all * 2);
      if (it % 2) {
        const int mode = rnd(0, 4);
        perturb(nl, ch.data() + (size_t)b * n_all * 2, mode);
        clean = clean && mode == 4;
      }
      if (it % 16 == 3 && nl >= 4) {  // a cycle: a node lists its ancestor, the root
        ch[(size_t)b * n_all * 2 + 2 * nl] = n_all - 1;
        clean = false;
      }
    }
    const int64_t per = 4LL * n_all + 4LL * ni;
    const int64_t n = trex_spr_plan_ints(B, n_all);
    if (n != TREX_PLAN_HEADER_INTS + B * per) return 26;
    std::vector<int32_t> plan((size_t)n), nni((size_t)trex_nni_plan_ints(B, n_all));
    const int rc = trex_spr_plan_build(ch.data(), B, n_all, plan.data());
    if (rc != 0 && rc != TREX_E_TOPOLOGY && rc != TREX_E_ARG) return 27;
    if (rc != trex_nni_plan_build(ch.data(), B, n_all, nni.data())) return 28;  // same rule
    if (clean && nl >= 3 && rc != 0) return 29;
    if (nl < 3 && rc == 0) return 30;
    if (rc != 0) {
      ++refused;
      continue;
    }
    ++built;
    for (int b = 0; b < B; ++b) {
      const int32_t* node = plan.data() + TREX_PLAN_HEADER_INTS + (size_t)b * per;
      const int32_t* walk = node + 4 * n_all;
      if (node[4 * (n_all - 1)] != -1 || node[4 * (n_all - 1) + 1] != -1 ||
          node[4 * (n_all - 1) + 2] != 0 || node[4 * (n_all - 1) + 3] != n_all)
        return 31;
      for (int x = 0; x < n_all - 1; ++x) {
        const int32_t* r = node + 4 * x;
        if (r[0] <= x || r[0] < nl || r[0] >= n_all || r[1] < 0 || r[1] >= n_all || r[1] == x)
          return 32;
        const int32_t* p = node + 4 * r[0];
        const int32_t* s = node + 4 * r[1];
        if (s[0] != r[0] || s[1] != x) return 33;
        if (r[2] <= p[2] || r[3] > p[3] || r[3] <= r[2] || (x < nl && r[3] != r[2] + 1)) return 34;
        if (r[3] != s[2] && s[3] != r[2]) return 35;  // the two intervals share a border
      }
      std::vector<int> seen(ni, 0);
      int last = -1;
      for (int k = 0; k < ni; ++k) {
        const int32_t* w = walk + 4 * k;
        if (w[0] < 0 || w[0] >= ni || seen[w[0]]++ || w[3] != 0) return 36;
        const int x = nl + w[0];
        if (node[4 * x + 2] <= last) return 37;  // ascending entry
        last = node[4 * x + 2];
        for (int c = 1; c <= 2; ++c)
          if (w[c] < 0 || w[c] >= x || node[4 * w[c]] != x) return 38;
      }
    }
  }
  std::printf("spr plans: %d built, %d refused\n", built, refused);
  return 0;
}

int check_ragged() {
  for (int it = 0; it < 200; ++it) {
    const int B = rnd(1, 8);
    std::vector<int32_t> n_all(B), L(B);
    size_t tot = 0;
    for (int b = 0; b < B; ++b) {
      n_all[b] = 2 * rnd(2, 70) - 1;
      L[b] = rnd(1, 700);
      tot += (size_t)n_all[b] * 2;
    }
    std::vector<int32_t> ch(tot);
    size_t off = 0;
    for (int b = 0; b < B; ++b) {
      const int nl = (n_all[b] + 1) / 2;
      random_tree(nl, ch.data() + off);
      if (it % 3 == 0) perturb(nl, ch.data() + off, rnd(0, 4));
      off += (size_t)n_all[b] * 2;
    }
    const int64_t n = trex_ragged_plan_ints(B, n_all.data(), L.data());
    if (n <= 0) return 2;
    std::vector<int32_t> plan((size_t)n);
    int64_t info[8];
    const int rc = trex_ragged_plan_build(ch.data(), n_all.data(), L.data(), B, plan.data(), info);
    if (rc != 0 && rc != TREX_E_TOPOLOGY && rc != TREX_E_ARG) return 3;
  }
  std::printf("ragged plans: 200\n");
  return 0;
}

int check_cpu_port() {
  for (int it = 0; it < 24; ++it) {
    const int nl = rnd(2, 40);
    const int n_all = 2 * nl - 1;
    const int B = rnd(1, 3);
    const int L = rnd(1, 300);
    const int Q = rnd(2, 20);
    const float tau = (it % 2) ? 0.0f : 0.5f;
    std::vector<int32_t> ch((size_t)B * n_all * 2);
    for (int b = 0; b < B; ++b) random_tree(nl, ch.data() + (size_t)b * n_all * 2);
    std::vector<int8_t> leaves((size_t)B * nl * L);
    for (auto& x : leaves) x = (int8_t)rnd(-1, Q);  // -1 / Q: missing (all-1e5 row)
    std::vector<float> cost((size_t)Q * Q);
    for (int i = 0; i < Q; ++i)
      for (int j = 0; j < Q; ++j) cost[(size_t)i * Q + j] = i == j ? 0.0f : (float)rnd(1, 4);
    const int ni = n_all - nl;
    std::vector<float> dp((it % 3) ? (size_t)B * ni * Q * L : 0);
    std::vector<double> ts(B), dc((size_t)Q * Q);
    const int rc = sankoff_cpu_fwd_bwd(ch.data(), leaves.data(), cost.data(), B, L, n_all, Q, tau,
                                       dp.empty() ? nullptr : dp.data(), ts.data(), dc.data(),
                                       1, 2);
    if (rc != 0) return 4;
  }
  std::printf("cpu port runs: 24\n");
  return 0;
}

}  // namespace

int main() {
  if (int e = check_uniform()) return e;
  if (int e = check_ragged()) return e;
  if (int e = check_cpu_port()) return e;
  if (int e = check_nni()) return e;
  if (int e = check_attach()) return e;
  if (int e = check_spr()) return e;
  std::printf("sanitize ok\n");
  return 0;
}
