"""SPR neighbour scoring at the C4 shape: the forward, outside and SPR passes
against what they replace, one forward per neighbour.

    python tools/time_spr.py [--trees 1024] [--taxa 32] [--sites 5000] [--states 4]
                             [--window 0.5] [--out FILE]

Timed as tools/time_nni.py does (device events around windows of >= --window
seconds after the clocks have settled).  Per tau (0 and 0.5) one JSON line:
forward_ms, outside_ms, spr_ms, the count of finite entries (the moves that
exist, the identity entries (v, sibling(v)) included) and bruteforce_ms = that
count per tree x the engine's own forward of the same trees, measured in the
same run (every neighbour scored as a tree of its own), and the workspace
bytes.  As information only: the wall time of one spr_hill_climb and one
nni_hill_climb from the same random trees on one alignment, which includes the
per-round plan rebuilds on the host, and the scores they reach.
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
from time_nni import settle, window_ms  # noqa: E402
from trex_amd import SankoffEngine, lib, nni_hill_climb, spr_hill_climb  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=1024)
    ap.add_argument("--taxa", type=int, default=32)
    ap.add_argument("--sites", type=int, default=5000)
    ap.add_argument("--states", type=int, default=4)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--climb-trees", type=int, default=64,
                    help="trees of the hill-climb wall times (0: skip them)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, n, L, Q = a.trees, a.taxa, a.sites, a.states
    ch, plan, leaves, cost = bench.make_inputs(torch, dev, B, n, L, Q, 0, B)
    eng = SankoffEngine(plan, L, Q, dev)
    n_all = plan.n_all
    ws_bytes = int(lib().trex_spr_workspace_bytes(B, L, n_all, Q))
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
        t_o, n_o = window_ms(lambda: eng.outside(leaves, cost, tau, f.dp), a.window)
        spr = eng.spr_scores(leaves, cost, tau, dp=f.dp, outside=out)
        finite = int(torch.isfinite(spr).sum())
        t_s, n_s = window_ms(lambda: eng.spr_scores(leaves, cost, tau, dp=f.dp, outside=out),
                             a.window)
        brute = finite / B * t_f  # one forward of the batch scores one neighbour of every tree
        total = t_f + t_o + t_s
        lines.append({
            "tool": "time_spr", "device": torch.cuda.get_device_name(0),
            "shape": {"trees": B, "taxa": n, "sites": L, "states": Q}, "tau": tau,
            "entries_per_tree": (n_all - 1) * n_all, "finite_entries_per_tree": finite / B,
            "settle_forwards": settled, "window_s": a.window,
            "calls": {"forward": n_f, "outside": n_o, "spr": n_s},
            "forward_ms": round(t_f, 4), "outside_ms": round(t_o, 4), "spr_ms": round(t_s, 4),
            "forward_outside_spr_ms": round(total, 4),
            "bruteforce_ms": round(brute, 3),
            "spr_speedup_vs_bruteforce": round(brute / t_s, 2),
            "speedup_vs_bruteforce": round(brute / total, 2),
            "faster_than_bruteforce": bool(t_s < brute),
            "spr_over_outside": round(t_s / t_o, 2),
            "workspace_bytes": ws_bytes,
        })
    if a.climb_trees > 0:  # information only: whole climbs, host work included
        k = min(a.climb_trees, B)
        align = leaves[0].contiguous()
        walls = {}
        for name, climb in (("spr", spr_hill_climb), ("nni", nni_hill_climb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = climb(ch[:k], align, cost, device=dev)
            torch.cuda.synchronize()
            walls[name] = (time.perf_counter() - t0, res)
        for line in lines:
            line["climb_trees"] = k
            for name, (wall, res) in walls.items():
                line[f"{name}_hill_climb_wall_s"] = round(wall, 3)
                line[f"{name}_hill_climb_rounds"] = int(res.rounds)
                line[f"{name}_hill_climb_mean_score"] = float(res.scores.mean())
    for line in lines:
        print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")
    if not all(x["faster_than_bruteforce"] for x in lines):
        sys.exit("spr_ms is not below bruteforce_ms")


if __name__ == "__main__":
    main()
