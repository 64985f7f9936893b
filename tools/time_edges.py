"""Per-branch change counts at the C4 shape: the edge pass next to the forward,
outside and attach passes of the same run.

    python tools/time_edges.py [--trees 1024] [--taxa 32] [--sites 5000] [--states 4]
                               [--window 0.5] [--weights] [--out FILE]

Timed as tools/time_nni.py does (device events around windows of >= --window
seconds after the clocks have settled).  Per tau (0 and 0.5) one JSON line:
forward_ms, outside_ms, attach_ms, backtrack_ms (tau = 0: the reconstruction
the counts follow) and edges_ms = one SankoffEngine.edge_changes call on given
tables and states (the edge kernel and its two reduce kernels), the bytes the
call moves by the shapes (what the attach pass reads plus the states, and the
fp64 partials written and read once) and the rate that gives, and the
workspace bytes.  --weights adds edges_w_ms, the call with site weights.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from time_nni import settle, window_ms  # noqa: E402
from trex_amd import SankoffEngine, lib  # noqa: E402


def edge_bytes(plan, L, Q, hard):
    """Bytes of one edge_changes call by the shapes: per internal row its
    outside row and its two children's inside rows (Q floats per site; a leaf
    child is its 1-byte code), at tau = 0 the int8 states of the row and of
    its internal children, the fp64 partials written once and read once, the
    tiles' totals written and read once more, the fp32 outputs."""
    nl, ni, B, n_all = plan.n_leaves, plan.n_int, plan.B, plan.n_all
    row = 4 * Q
    kids = plan.children[:, nl:, :]
    kids_leaf = int((kids < nl).sum())
    kids_int = B * ni * 2 - kids_leaf
    tiles = (L + 63) // 64
    E = Q * Q + (2 if hard else 0)
    tables = L * (B * ni * row + kids_int * row + kids_leaf)
    states = L * (B * ni + kids_int) if hard else 0
    partials = B * tiles * (n_all - 1) * E * 8 * 2 + B * n_all * E * 8 * 2
    return tables + states + partials + B * n_all * (E + 1) * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=1024)
    ap.add_argument("--taxa", type=int, default=32)
    ap.add_argument("--sites", type=int, default=5000)
    ap.add_argument("--states", type=int, default=4)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--weights", action="store_true", help="also time the weighted call")
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
    ws_bytes = int(lib().trex_edge_workspace_bytes(B, L, plan.n_all, Q))
    lines = []
    settled = None
    for tau in (0.0, 0.5):
        hard = tau == 0.0
        f = eng.forward(leaves, cost, tau)
        out = eng.outside(leaves, cost, tau, f.dp)
        o = {"dp": f.dp, "tree_score": f.tree_score}
        fwd = lambda: eng.forward(leaves, cost, tau, out=o)  # noqa: E731
        if settled is None:
            settled = settle(fwd)
        t_f, n_f = window_ms(fwd, a.window)
        t_o, n_o = window_ms(lambda: eng.outside(leaves, cost, tau, f.dp), a.window)
        t_a, n_a = window_ms(lambda: eng.attach_scores(leaves, cost, tau, new_leaf=new, dp=f.dp,
                                                       outside=out), a.window)
        states, t_b, n_b = None, None, 0
        if hard:
            states = eng.backtrack(cost, f.dp)
            t_b, n_b = window_ms(lambda: eng.backtrack(cost, f.dp), a.window)
        edges = lambda wt: eng.edge_changes(leaves, cost, tau, dp=f.dp, outside=out,  # noqa: E731
                                            states=states, weights=wt)
        r = edges(None)
        t_e, n_e = window_ms(lambda: edges(None), a.window)
        nbytes = edge_bytes(plan, L, Q, hard)
        line = {
            "tool": "time_edges", "device": torch.cuda.get_device_name(0),
            "shape": {"trees": B, "taxa": n, "sites": L, "states": Q}, "tau": tau,
            "edges_per_tree": plan.n_all - 1, "settle_forwards": settled, "window_s": a.window,
            "calls": {"forward": n_f, "outside": n_o, "attach": n_a, "backtrack": n_b,
                      "edges": n_e},
            "forward_ms": round(t_f, 4), "outside_ms": round(t_o, 4), "attach_ms": round(t_a, 4),
            "backtrack_ms": None if t_b is None else round(t_b, 4),
            "edges_ms": round(t_e, 4), "edges_over_attach": round(t_e / t_a, 2),
            "edges_bytes": nbytes, "edges_TBps": round(nbytes / (t_e * 1e-3) / 1e12, 3),
            "workspace_bytes": ws_bytes,
            "mean_tree_length": float(r.lengths.sum(dim=1).mean()),
            "mean_tree_score": float(f.tree_score.mean()),
        }
        if w is not None:
            t_w, n_w = window_ms(lambda: edges(w), a.window)
            line["calls"]["edges_w"] = n_w
            line["edges_w_ms"] = round(t_w, 4)
        lines.append(line)
    for line in lines:
        print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
