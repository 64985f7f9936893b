"""Generate tests/golden fixtures (run from the repo root).

The reference (JAX) cannot be imported in this image, so the fixtures are:
  * kat_sankoff.json -- hand-derived known answers on the reference's own test
    fixtures (tests/test_sankoff.py:9-72; derivation in SURVEY.md §4) and the
    tie-averaged gradient derived by hand for the same tree;
  * sankoff_cases.npz -- oracle outputs on seeded inputs, pinned so later
    oracle edits cannot drift silently (tests/test_oracle.py re-derives them);
  * plan_cases.npz -- what the built library's host planner returns on a
    corpus of child lists (needs libtrexhip.so; `plan` writes this one alone).

    python tests/golden/make_golden.py [plan]
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from _cases import (balanced_children, int_cost, random_leaves, random_topologies,  # noqa: E402
                    weird_children)
from oracle.sankoff_ref import run_sankoff_ref  # noqa: E402
from oracle.softmin_ref import batched_fwd_bwd_ref  # noqa: E402
from trex_amd.topology import adjacency_from_children  # noqa: E402

KAT = {
    "source": "reference tests/test_sankoff.py:39-72 fixture; values hand-derived",
    "adjacency_edges": [[0, 3], [1, 3], [2, 4], [3, 4]],
    "cost": [[0, 1], [1, 0]],
    "leaf_sequences": [[0, 1], [1, 0], [0, 0]],
    "n_all": 5, "n_states": 2, "n_leaves": 3,
    "total": 2.0,
    "dp": [[[0, 1e5], [1e5, 0], [0, 1e5], [1, 1], [1, 2]],
           [[1e5, 0], [0, 1e5], [0, 1e5], [1, 1], [1, 2]]],
    "reconstructed": [[0, 1], [1, 0], [0, 0], [0, 0], [0, 0]],
    # d total / d cost (tie-averaged, hard): root argmin state 0 at both
    # sites; every message picks a unique argmin; see DESIGN.md "KAT".
    "d_cost": [[6, 2], [0, 0]],
    # the same fixture under an asymmetric matrix, C[parent][child]
    # (sankoff.py:67-68, min(cost_matrix + dp[child], axis=1)), by hand:
    # node 3 = (0, 1): D3[i] = C[i][0] + C[i][1] = [3, 4] at both sites (the
    # leaves are 0, 1 and 1, 0); node 4 = (2, 3), leaf 2 = 0: D4[i] = C[i][0]
    # + min_j (C[i][j] + D3[j]) = [1 + min(4, 6), 4 + min(7, 4)] = [5, 8];
    # total 2 * 5; root 0, node 3 argmin_j (C[0][j] + D3[j]) = 0; per site the
    # edges charge C[0][0] three times (leaf 2, node 3, leaf 0 | 1) and
    # C[0][1] once.  Under C^T: D3 = [5, 2], D4 = [1 + 6, 2 + 2] = [7, 4],
    # total 8, root and node 3 in state 1.
    "asymmetric": {
        "cost": [[1, 2], [4, 0]],
        "total": 10.0,
        "dp": [[[0, 1e5], [1e5, 0], [0, 1e5], [3, 4], [5, 8]],
               [[1e5, 0], [0, 1e5], [0, 1e5], [3, 4], [5, 8]]],
        "reconstructed": [[0, 1], [1, 0], [0, 0], [0, 0], [0, 0]],
        "d_cost": [[6, 2], [0, 0]],
        "transposed": {
            "total": 8.0,
            "dp": [[[0, 1e5], [1e5, 0], [0, 1e5], [5, 2], [7, 4]],
                   [[1e5, 0], [0, 1e5], [0, 1e5], [5, 2], [7, 4]]],
            "reconstructed": [[0, 1], [1, 0], [0, 0], [1, 1], [1, 1]],
        },
    },
    "run_dp_fixture": {
        "source": "reference tests/test_sankoff.py:9-36",
        "adjacency": [[0, 1, 0], [0, 1, 0], [0, 0, 0]],
        "sequences": [[0], [1], [0]],
        "dp": [[0, 1e5], [1e5, 0], [2e5, 2e5]],
        "bt_row2": [[-1, 0, -1, 0], [-1, 1, -1, 1]],
    },
}


def cases():
    out = {}
    k = 0
    for n, L, Q in [(8, 37, 4), (16, 64, 3), (12, 50, 2)]:
        ch = random_topologies(2, n, seed=10 + k)
        leaves = random_leaves(2, n, L, Q, seed=20 + k, missing=0.05)
        cost = int_cost(Q, seed=30 + k)
        out[f"c{k}"] = (ch, leaves, cost)
        k += 1
    for case in ("fwdref", "dag"):
        ch = weird_children(case)[None]
        leaves = random_leaves(1, 8, 40, 4, seed=40 + k)
        out[case] = (ch, leaves, int_cost(4, seed=50 + k))
        k += 1
    return out


def compute(ch, leaves, cost):
    res = {}
    hard = batched_fwd_bwd_ref(ch, leaves, cost, 0.0)
    soft = batched_fwd_bwd_ref(ch, leaves, cost, 0.5)
    res["hard_dp"] = hard["dp"].astype(np.float32)
    res["hard_tree_score"] = hard["tree_score"]
    res["hard_d_cost"] = hard["d_cost"]
    res["soft_tree_score"] = soft["tree_score"]
    res["soft_d_cost"] = soft["d_cost"]
    adj = adjacency_from_children(ch)
    n_all = ch.shape[1]
    nl = (n_all + 1) // 2
    recon = []
    for b in range(ch.shape[0]):
        r = run_sankoff_ref(adj[b], cost, leaves[b].astype(np.float32), n_all, cost.shape[0],
                            nl, return_path=True)
        recon.append(r[0])
    res["recon"] = np.stack(recon)
    return res


def plan_corpus():
    """Child lists for the planner fixture: uniform batches by name, and
    ragged batches by name as (list of per-tree child lists, site counts)."""
    u = {f"random{nl}": random_topologies(3, nl, seed=nl) for nl in (3, 4, 8, 16, 40, 64)}
    u["balanced64"] = balanced_children(64, B=2)
    n = 33  # a caterpillar: every internal child is the previous step
    cat = np.full((1, 2 * n - 1, 2), -1, np.int32)
    cat[0, n] = (0, 1)
    for k in range(1, n - 1):
        cat[0, n + k] = (k + 1, n + k - 1)
    u["caterpillar33"] = cat
    for kind in ("fwdref", "dag", "cycle"):
        u[kind] = weird_children(kind)[None]
    # test_plan_deferred_cherries' tree: 13 an orphan, cherry 10 with two parents
    u["unreached"] = balanced_children(8).copy()
    u["unreached"][0, 14] = (12, 10)
    # row 8 a child of 11 and of 12, every row reached (leaf 7 is unused)
    u["shared"] = balanced_children(8).copy()
    u["shared"][0, 11] = (6, 8)
    u["n_all3"] =np.array([[[-1, -1], [-1, -1], [0, 1]]], np.int32)  # 2 leaves
    u["n_all4"] = np.array([[[-1, -1], [-1, -1], [0, 1], [1, 2]]], np.int32)  # even
    u["malformed"] = balanced_children(8).copy()
    u["malformed"][0, 9, 0] = 99
    r = {
        "a": ([u["random3"][0], u["random8"][1], u["random40"][2], u["fwdref"][0],
               u["balanced64"][0]], [1, 64, 65, 7, 130]),
        "b": ([u["dag"][0], u["cycle"][0], u["unreached"][0], u["caterpillar33"][0],
               u["n_all3"][0], u["random16"][0], u["random64"][0]],
              [65, 1, 64, 200, 5, 64, 1000]),
        "malformed": ([u["random4"][0], u["malformed"][0]], [3, 3]),
        "no_sites": ([u["random4"][0]], [0]),
    }
    return u, r


def plan_main():
    """plan_cases.npz: the host planner's output (trex_amd/csrc/plan.cpp) on
    the corpus above, with TREX_DEFER unset and "0".  It pins the plan format
    bit for bit: regenerate it only with a deliberate format change (and a
    trex_version() bump).  tests/test_plan_golden_cpu.py rebuilds every case."""
    from _plan_golden import ints_table, run_ragged, run_uniform

    uniform, ragged = plan_corpus()
    arrays = {"ints": ints_table()}
    for name, ch in uniform.items():
        arrays[f"u/{name}/children"] = ch
        for defer in (True, False):
            for key, val in run_uniform(ch, defer).items():
                arrays[f"u/{name}/{'defer' if defer else 'nodefer'}/{key}"] = val
    for name, (trees, sites) in ragged.items():
        arrays[f"r/{name}/children"] = np.concatenate(trees, axis=0)
        arrays[f"r/{name}/n_all"] = np.array([len(t) for t in trees], np.int32)
        arrays[f"r/{name}/sites"] = np.array(sites, np.int32)
        for defer in (True, False):
            out = run_ragged(arrays[f"r/{name}/children"], arrays[f"r/{name}/n_all"],
                             arrays[f"r/{name}/sites"], defer)
            for key, val in out.items():
                arrays[f"r/{name}/{'defer' if defer else 'nodefer'}/{key}"] = val
    np.savez_compressed(os.path.join(HERE, "plan_cases.npz"), **arrays)
    print("wrote plan_cases.npz:", len(uniform), "uniform,", len(ragged), "ragged batches")


def main():
    if sys.argv[1:] == ["plan"]:  # the planner fixture alone
        return plan_main()
    plan_main()
    with open(os.path.join(HERE, "kat_sankoff.json"), "w") as f:
        json.dump(KAT, f, indent=1)
    arrays = {}
    for name, (ch, leaves, cost) in cases().items():
        arrays[f"{name}/children"] = ch
        arrays[f"{name}/leaves"] = leaves
        arrays[f"{name}/cost"] = cost
        for key, val in compute(ch, leaves, cost).items():
            arrays[f"{name}/{key}"] = val
    np.savez_compressed(os.path.join(HERE, "sankoff_cases.npz"), **arrays)
    print("wrote", sorted(set(k.split("/")[0] for k in arrays)))


if __name__ == "__main__":
    main()
