"""Attachment scoring at the C4 shape: the outside pass and the attach kernel
against what they replace, one forward per candidate edge.

    python tools/time_attach.py [--trees 1024] [--taxa 32] [--sites 5000] [--states 4]
                                [--window 0.5] [--weights] [--out FILE]

Timed as tools/time_nni.py does (device events around windows of >= --window
seconds after the clocks have settled).  Per tau (0 and 0.5) one JSON line:
forward_ms, outside_ms, attach_ms, bruteforce_ms = n_edges x the measured
forward of the (taxa + 1)-taxon trees (every candidate scored as a tree of its
own, in the same run), the bytes each pass moves by the shapes (no cache reuse
assumed) and the bytes/s that gives.  As information only: the wall time of
one stepwise_addition with --trees addition sequences of --taxa taxa, which
includes the per-step plan rebuilds on the host.  --weights also times
attach_scores with uniform(0.25, 2) site weights next to the unweighted call:
attach_weighted_ms and weighted_over_unweighted.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from time_nni import pass_bytes, settle, window_ms  # noqa: E402
from trex_amd import SankoffEngine, TreePlan, random_topologies, stepwise_addition  # noqa: E402


def attach_bytes(plan, L, Q):
    """Bytes of the attach pass by the shapes: per internal row its outside
    row and its two children's inside rows (Q floats per site; a leaf child is
    its 1-byte code), the root's DP row once more, the new leaf's code, and
    the fp64 partials written and read once."""
    nl, ni, B = plan.n_leaves, plan.n_int, plan.B
    row = 4 * Q
    kids = plan.children[:, nl:, :]
    kids_leaf = int((kids < nl).sum())
    kids_int = B * ni * 2 - kids_leaf
    tiles = (L + 63) // 64
    return (L * (B * ni * row + kids_int * row + kids_leaf + B * row + B)
            + B * tiles * plan.n_all * 8 * 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=1024)
    ap.add_argument("--taxa", type=int, default=32)
    ap.add_argument("--sites", type=int, default=5000)
    ap.add_argument("--states", type=int, default=4)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--weights", action="store_true",
                    help="also time the weighted call (trex_sankoff_attach_w)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, n, L, Q = a.trees, a.taxa, a.sites, a.states
    ch, plan, leaves, cost = bench.make_inputs(torch, dev, B, n, L, Q, 0, B)
    eng = SankoffEngine(plan, L, Q, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(6)
    new = torch.randint(0, Q, (B, L), generator=g, device=dev, dtype=torch.int8)
    w = torch.rand((B, L), generator=g, device=dev) * 1.75 + 0.25 if a.weights else None
    # the grown trees a forward per edge would score: n + 1 taxa
    big = SankoffEngine(TreePlan(random_topologies(B, n + 1, seed=4)), L, Q, dev)
    big_leaves = torch.cat([leaves, new[:, None]], dim=1).contiguous()
    n_edges = 2 * n - 1
    b_out, _ = pass_bytes(plan, L, Q)
    b_att = attach_bytes(plan, L, Q)
    lines = []
    settled = None
    for tau in (0.0, 0.5):
        f = eng.forward(leaves, cost, tau)
        out = eng.outside(leaves, cost, tau, f.dp)
        o = {"dp": f.dp, "tree_score": f.tree_score}
        fwd = lambda: eng.forward(leaves, cost, tau, out=o)  # noqa: E731
        if settled is None:
            settled = settle(fwd)
        t_f, n_f = window_ms(fwd, a.window)
        fb = big.forward(big_leaves, cost, tau)
        ob = {"dp": fb.dp, "tree_score": fb.tree_score}
        t_b, n_b = window_ms(lambda: big.forward(big_leaves, cost, tau, out=ob), a.window)
        t_o, n_o = window_ms(lambda: eng.outside(leaves, cost, tau, f.dp), a.window)
        t_a, n_a = window_ms(lambda: eng.attach_scores(leaves, cost, tau, new_leaf=new, dp=f.dp,
                                                       outside=out), a.window)
        brute = n_edges * t_b
        line = {
            "tool": "time_attach", "device": torch.cuda.get_device_name(0),
            "shape": {"trees": B, "taxa": n, "sites": L, "states": Q}, "tau": tau,
            "edges_per_tree": n_edges, "settle_forwards": settled, "window_s": a.window,
            "calls": {"forward": n_f, "forward_grown": n_b, "outside": n_o, "attach": n_a},
            "forward_ms": round(t_f, 4), "forward_grown_ms": round(t_b, 4),
            "outside_ms": round(t_o, 4), "attach_ms": round(t_a, 4),
            "bruteforce_ms": round(brute, 3),
            "outside_plus_attach_ms": round(t_o + t_a, 4),
            "speedup_vs_bruteforce": round(brute / (t_o + t_a), 2),
            "faster_than_bruteforce": bool(t_o + t_a < brute),
            "outside_bytes": b_out, "attach_bytes": b_att,
            "outside_TBps": round(b_out / (t_o * 1e-3) / 1e12, 3),
            "attach_TBps": round(b_att / (t_a * 1e-3) / 1e12, 3),
        }
        if w is not None:
            t_w, n_w = window_ms(lambda: eng.attach_scores(leaves, cost, tau, new_leaf=new,
                                                           dp=f.dp, outside=out, weights=w),
                                 a.window)
            line["calls"]["attach_weighted"] = n_w
            line["attach_weighted_ms"] = round(t_w, 4)
            line["weighted_over_unweighted"] = round(t_w / t_a, 4)
        lines.append(line)
    # information only: one whole stepwise addition, host work included
    align = leaves[0].contiguous()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = stepwise_addition(align, cost, n_trees=B, seed=0, device=dev)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    for line in lines:
        line["stepwise_addition_wall_s"] = round(wall, 3)
        line["stepwise_addition_best_score"] = float(res.scores.min())
        print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")
    if not all(x["faster_than_bruteforce"] for x in lines):
        sys.exit("outside_ms + attach_ms is not below bruteforce_ms")


if __name__ == "__main__":
    main()
