"""NNI neighbour scoring at the C4 shape: the outside pass and the scoring
kernel against what they replace, one forward per neighbour.

    python tools/time_nni.py [--trees 1024] [--taxa 32] [--sites 5000] [--states 4]
                             [--window 0.5] [--weights] [--out FILE]

Device events around windows of >= --window seconds of back-to-back launches,
after the clocks have settled (blocks of forwards until one is within 1 % of
the one before, as bench.py does) and a warm-up of every kernel.  Per tau
(0 and 0.5) one JSON line: forward_ms, outside_ms, nni_ms, bruteforce_ms =
n_neighbours x forward_ms (the forward kernel scoring every neighbour as a
tree of its own, measured in the same run), the bytes each pass moves by the
shapes (no cache reuse assumed) and the bytes/s that gives.  --weights also
times nni_scores with uniform(0.25, 2) site weights next to the unweighted
call: nni_weighted_ms and weighted_over_unweighted.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from trex_amd import SankoffEngine  # noqa: E402


def window_ms(fn, seconds):
    """ms per call over one event-bracketed window of >= `seconds`."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    n = max(3, int(math.ceil(seconds / max(e0.elapsed_time(e1) * 1e-3, 1e-6))))
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, n


def settle(fn):
    """Blocks of >= 50 ms of fn until one is within 1 % of the one before."""
    prev, blocks = None, 0
    per, _ = window_ms(fn, 0.0)
    nblk = max(5, int(math.ceil(50.0 / max(per, 1e-3))))
    for blocks in range(1, 21):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(nblk):
            fn()
        e1.record()
        torch.cuda.synchronize()
        cur = e0.elapsed_time(e1) / nblk
        if prev is not None and cur >= 0.99 * prev:
            break
        prev = cur
    return blocks * nblk


def pass_bytes(plan, L, Q):
    """(outside, nni) bytes by the shapes: rows are Q floats per site, a leaf
    child is its 1-byte code; every access counted once, no cache reuse."""
    tab = plan.nni_table.astype("int64")  # (B, n_int - 1, 4): u, a0, a1, s
    nl, ni, B = plan.n_leaves, plan.n_int, plan.B
    row = 4 * Q
    sib_leaf = int((tab[:, :, 3] < nl).sum())
    sib_int = B * (ni - 1) - sib_leaf
    outside = L * (B * ni * row  # every outside row written
                   + B * (ni - 1) * row  # the parent's outside row read
                   + sib_int * row + sib_leaf)  # the sibling's inside row
    kids_leaf = int((tab[:, :, 1:] < nl).sum())
    kids_int = B * (ni - 1) * 3 - kids_leaf
    tiles = (L + 63) // 64
    nni = L * (B * (ni - 1) * row + kids_int * row + kids_leaf) + B * tiles * (ni - 1) * 2 * 8 * 2
    return outside, nni


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=1024)
    ap.add_argument("--taxa", type=int, default=32)
    ap.add_argument("--sites", type=int, default=5000)
    ap.add_argument("--states", type=int, default=4)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--weights", action="store_true",
                    help="also time the weighted call (trex_sankoff_nni_w)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, n, L, Q = a.trees, a.taxa, a.sites, a.states
    ch, plan, leaves, cost = bench.make_inputs(torch, dev, B, n, L, Q, 0, B)
    eng = SankoffEngine(plan, L, Q, dev)
    n_nb = 2 * (n - 2)
    b_out, b_nni = pass_bytes(plan, L, Q)
    w = None
    if a.weights:
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        w = torch.rand((B, L), generator=g, device=dev) * 1.75 + 0.25
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
        t_n, n_n = window_ms(lambda: eng.nni_scores(leaves, cost, tau, dp=f.dp, outside=out),
                             a.window)
        brute = n_nb * t_f
        line = {
            "tool": "time_nni", "device": torch.cuda.get_device_name(0),
            "shape": {"trees": B, "taxa": n, "sites": L, "states": Q}, "tau": tau,
            "neighbours_per_tree": n_nb, "settle_forwards": settled,
            "window_s": a.window, "calls": {"forward": n_f, "outside": n_o, "nni": n_n},
            "forward_ms": round(t_f, 4), "outside_ms": round(t_o, 4), "nni_ms": round(t_n, 4),
            "bruteforce_ms": round(brute, 3),
            "outside_plus_nni_ms": round(t_o + t_n, 4),
            "speedup_vs_bruteforce": round(brute / (t_o + t_n), 2),
            "faster_than_bruteforce": bool(t_o + t_n < brute),
            "outside_bytes": b_out, "nni_bytes": b_nni,
            "outside_TBps": round(b_out / (t_o * 1e-3) / 1e12, 3),
            "nni_TBps": round(b_nni / (t_n * 1e-3) / 1e12, 3),
        }
        if w is not None:
            t_w, n_w = window_ms(lambda: eng.nni_scores(leaves, cost, tau, dp=f.dp, outside=out,
                                                        weights=w), a.window)
            line["calls"]["nni_weighted"] = n_w
            line["nni_weighted_ms"] = round(t_w, 4)
            line["weighted_over_unweighted"] = round(t_w / t_n, 4)
        print(json.dumps(line))
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")
    if not all(x["faster_than_bruteforce"] for x in lines):
        sys.exit("outside_ms + nni_ms is not below bruteforce_ms")


if __name__ == "__main__":
    main()
