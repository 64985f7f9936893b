"""State-set leaves against leaf codes at the C4 shape: forward, outside, NNI
and attachment scores of both encodings in one run on one device.

    python tools/time_sets.py [--trees 1024] [--taxa 32] [--sites 5000] [--states 4]
                              [--window 0.3] [--repeats 3] [--out FILE]

The sets path gets the singleton masks of the same leaves, so both encodings
compute the same tables.  Device events around windows of >= --window seconds
of back-to-back launches, after the clocks have settled (blocks of forwards
until one is within 1 % of the one before, as bench.py does) and a warm-up of
every kernel.  Every pass is timed --repeats times, the two encodings taking
turns, so a drift of the clocks hits both; the figure of a pass is the median
of its windows and ``spread`` their (max - min) / median, the same-run
run-to-run spread a ratio has to exceed to mean anything.  Per tau (0 and 0.5)
one JSON line: the ms of the four passes per encoding, sets / codes ratios, the
ratio of a search round (forward + outside + NNI), and the byte ratios the
shapes give (rows are Q floats per site, a leaf child its 1-byte code or
4-byte mask; every access counted once, no cache reuse).
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from trex_amd import SankoffEngine  # noqa: E402

PASSES = ("forward", "outside", "nni", "attach")


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


def pass_bytes(plan, L, Q, leaf, fwd_rereads):
    """Bytes of the four passes by the shapes for a leaf cell of `leaf` bytes.
    fwd_rereads: the forward reads an internal child's row back from the table
    (the state-set forward does; the code forward keeps rows on chip)."""
    tab = plan.nni_table.astype("int64")  # (B, n_int - 1, 4): u, a0, a1, s
    nl, ni, B = plan.n_leaves, plan.n_int, plan.B
    row = 4 * Q
    tiles = (L + 63) // 64
    forward = (L * B * (ni * row + (ni - 1) * row * int(fwd_rereads) + nl * leaf)
               + B * tiles * 8 * 2)
    sib_leaf = int((tab[:, :, 3] < nl).sum())
    sib_int = B * (ni - 1) - sib_leaf
    outside = L * (B * ni * row + B * (ni - 1) * row + sib_int * row + sib_leaf * leaf)
    kids_leaf = int((tab[:, :, 1:] < nl).sum())
    kids_int = B * (ni - 1) * 3 - kids_leaf
    nni = (L * (B * (ni - 1) * row + kids_int * row + kids_leaf * leaf)
           + B * tiles * (ni - 1) * 2 * 8 * 2)
    attach = (L * B * (ni * row + (ni - 1) * row + nl * leaf + row + leaf)
              + B * tiles * (nl + ni) * 8 * 2)
    return {"forward": forward, "outside": outside, "nni": nni, "attach": attach}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=1024)
    ap.add_argument("--taxa", type=int, default=32)
    ap.add_argument("--sites", type=int, default=5000)
    ap.add_argument("--states", type=int, default=4)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, n, L, Q = a.trees, a.taxa, a.sites, a.states
    ch, plan, codes, cost = bench.make_inputs(torch, dev, B, n, L, Q, 0, B)
    eng = SankoffEngine(plan, L, Q, dev)
    leaves = {"codes": codes,
              "sets": torch.bitwise_left_shift(torch.ones_like(codes, dtype=torch.int32),
                                               codes.to(torch.int32)).contiguous()}
    g = torch.Generator(device=dev)
    g.manual_seed(6)
    new_codes = torch.randint(0, Q, (B, L), generator=g, device=dev, dtype=torch.int8)
    new = {"codes": new_codes,
           "sets": torch.bitwise_left_shift(torch.ones_like(new_codes, dtype=torch.int32),
                                            new_codes.to(torch.int32)).contiguous()}
    bytes_of = {"codes": pass_bytes(plan, L, Q, 1, False),
                "sets": pass_bytes(plan, L, Q, 4, True)}
    lines = []
    settled = None
    for tau in (0.0, 0.5):
        fns = {}
        for enc in ("codes", "sets"):
            lv, nw = leaves[enc], new[enc]
            f = eng.forward(lv, cost, tau)
            out = eng.outside(lv, cost, tau, f.dp)
            o = {"dp": f.dp, "tree_score": f.tree_score}
            fns[enc] = {
                "forward": lambda lv=lv, o=o: eng.forward(lv, cost, tau, out=o),
                "outside": lambda lv=lv, f=f: eng.outside(lv, cost, tau, f.dp),
                "nni": lambda lv=lv, f=f, out=out: eng.nni_scores(lv, cost, tau, dp=f.dp,
                                                                  outside=out),
                "attach": lambda lv=lv, f=f, out=out, nw=nw: eng.attach_scores(
                    lv, cost, tau, new_leaf=nw, dp=f.dp, outside=out),
            }
        if settled is None:
            settled = settle(fns["codes"]["forward"])
        ms = {enc: {p: [] for p in PASSES} for enc in fns}
        for _ in range(a.repeats):
            for p in PASSES:
                for enc in ("codes", "sets"):
                    ms[enc][p].append(window_ms(fns[enc][p], a.window)[0])
        med = {enc: {p: statistics.median(ms[enc][p]) for p in PASSES} for enc in ms}
        spread = max((max(v) - min(v)) / statistics.median(v)
                     for enc in ms for v in ms[enc].values())
        rnd = {enc: med[enc]["forward"] + med[enc]["outside"] + med[enc]["nni"] for enc in med}
        line = {
            "tool": "time_sets", "device": torch.cuda.get_device_name(0),
            "shape": {"trees": B, "taxa": n, "sites": L, "states": Q}, "tau": tau,
            "settle_forwards": settled, "window_s": a.window, "repeats": a.repeats,
            "codes_ms": {p: round(med["codes"][p], 4) for p in PASSES},
            "sets_ms": {p: round(med["sets"][p], 4) for p in PASSES},
            "windows_ms": {enc: {p: [round(x, 4) for x in ms[enc][p]] for p in PASSES}
                           for enc in ms},
            "spread": round(spread, 4),
            "sets_over_codes": {p: round(med["sets"][p] / med["codes"][p], 4) for p in PASSES},
            "byte_ratio": {p: round(bytes_of["sets"][p] / bytes_of["codes"][p], 4)
                           for p in PASSES},
            "search_round_ms": {enc: round(rnd[enc], 4) for enc in rnd},
            "search_round_sets_over_codes": round(rnd["sets"] / rnd["codes"], 4),
        }
        print(json.dumps(line))
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
