"""The fused Q = 4 kernel's software pipelining (sankoff_fused4.hip: program
records and re-read rows loaded on the scalar pipe a step or two ahead, a
forward step's leaf codes read during the step before it, a reverse step's leaf
codes read once with its cotangent) against the generic one-wave fused kernel,
bit for bit.

As in test_fused4_gpu.py every case runs under TREX_WIDE_SMALLQ=0 and compares
the call with TREX_FUSED4 unset (the fused4 kernel, checked by its launch
counter) against TREX_FUSED4=0 (sankoff_kernel<4, true, 3>): dp, tree_score
and d_cost hold the same bytes.  The shapes are the smallest where the
pipelining can go wrong: 2 ... 8 internal nodes (every trip count modulo the
ring depth, prologues shorter than the ring, loads issued for steps before
record 0 and past the last one, a second tile with 4 live lanes), all-bypass
and all-slot chains, the non-symmetric body with missing codes, plans without
deferred steps, a workgroup holding items of two trees, the direct-softmin
branch, graph replay, and the guard-band protocol.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import _guard as G
from _cases import balanced_children, general_cost, hamming, random_leaves, random_topologies
from trex_amd import SankoffEngine, TreePlan
from trex_amd._lib import check, lib, ptr, stream_handle

pytestmark = pytest.mark.gpu

Q = 4


def pectinate(n):
    ch = np.full((2 * n - 1, 2), -1, dtype=np.int32)
    ch[n] = (0, 1)
    for k in range(1, n - 1):
        ch[n + k] = (k + 1, n + k - 1)
    return ch[None]


def shape_small(n):
    """3 random topologies of n taxa, 2 tiles each, the second with 4 live
    lanes; every fourth code on average missing"""
    return (random_topologies(3, n, seed=100 + n), random_leaves(3, n, 68, Q, seed=200 + n,
                                                                 missing=0.25),
            hamming(Q), 0.5, None)


def shape_32():
    """test_fused4_gpu.py's shape_b: asymmetric cost with a non-zero diagonal
    (the non-SYM body), 10 % missing codes, d_tree_score weights"""
    rng = np.random.default_rng(21)
    return (random_topologies(9, 32, seed=22), random_leaves(9, 32, 200, Q, seed=23, missing=0.1),
            general_cost(Q, 24, "asym_frac"), 0.7, rng.uniform(0.5, 2.0, 9).astype(np.float32))


def shape_straddle():
    """2 trees x 3 tiles: workgroup 0 holds tiles 0-2 of tree 0 and tile 0 of
    tree 1, workgroup 1 two items and two idle waves"""
    return (random_topologies(2, 13, seed=301), random_leaves(2, 13, 192, Q, seed=302, missing=0.1),
            general_cost(Q, 303, "asym_frac"), 0.6, None)


def _dev(x, device):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to(device).contiguous()


def _env(monkeypatch, fused4):
    monkeypatch.setenv("TREX_WIDE_SMALLQ", "0")
    if fused4:
        monkeypatch.delenv("TREX_FUSED4", raising=False)
    else:
        monkeypatch.setenv("TREX_FUSED4", "0")


def _call(eng, lv, c, tau, d):
    f, dc, _, _ = eng.fwd_bwd(lv, c, tau, d)
    torch.cuda.synchronize()
    return dict(dp=f.dp.clone(), tree_score=f.tree_score.clone(), d_cost=dc.clone())


def _compare(monkeypatch, device, ch, leaves, cost, tau, dts):
    _env(monkeypatch, True)
    eng = SankoffEngine(TreePlan(ch), leaves.shape[2], Q, device)
    assert eng.fused4_prog is not None
    lv, c, d = _dev(leaves, device), _dev(cost, device), _dev(dts, device)
    n0 = lib().trex_debug_fused4_launches()
    new = _call(eng, lv, c, tau, d)
    assert lib().trex_debug_fused4_launches() - n0 == 1
    _env(monkeypatch, False)
    old = _call(eng, lv, c, tau, d)
    assert lib().trex_debug_fused4_launches() - n0 == 1
    for k in old:
        G.assert_bitwise(new[k], old[k], f"{k}: TREX_FUSED4 unset vs 0")
    assert torch.isfinite(new["d_cost"]).all() and new["d_cost"].abs().sum() > 0
    return eng, (lv, c, d)


@pytest.mark.parametrize("n", range(3, 10))
def test_a_small_taxa_counts(monkeypatch, device, n):
    ch, leaves, cost, tau, dts = shape_small(n)
    assert ch.shape[1] == 2 * n - 1  # n - 1 = 2 ... 8 internal nodes
    _compare(monkeypatch, device, ch, leaves, cost, tau, dts)


@pytest.mark.parametrize("tree", ["pectinate", "balanced"])
def test_b_pectinate_and_balanced(monkeypatch, device, tree):
    """pectinate: every step hands on to the next one (bypass chains);
    balanced: every cotangent goes through a slot"""
    ch = pectinate(16) if tree == "pectinate" else balanced_children(16, B=1)
    leaves = random_leaves(1, 16, 64, Q, seed=311, missing=0.1)
    _compare(monkeypatch, device, ch, leaves, hamming(Q), 0.5, None)


def test_c_non_symmetric_body(monkeypatch, device):
    _compare(monkeypatch, device, *shape_32())


def test_d_no_deferred_steps(monkeypatch, device):
    """the plain cherry path reads its codes a step early"""
    monkeypatch.setenv("TREX_DEFER", "0")
    _compare(monkeypatch, device, *shape_32())


def test_e_workgroup_straddles_two_trees(monkeypatch, device):
    ch, leaves, cost, tau, dts = shape_straddle()
    tiles = (leaves.shape[2] + 63) // 64
    assert tiles == 3 and ch.shape[0] * tiles == 6
    _compare(monkeypatch, device, ch, leaves, cost, tau, dts)


def test_f_wide_range_cost_takes_the_direct_branch(monkeypatch, device):
    ch, leaves, _, _, dts = shape_straddle()
    cost = general_cost(Q, 41, "asym_wide")
    tau = 0.05
    assert (cost.max() - cost.min()) / tau > 40
    _compare(monkeypatch, device, ch, leaves, cost, tau, dts)


def test_g_captured_replay(monkeypatch, device):
    ch, leaves, cost, tau, dts = shape_straddle()
    eng, (lv, c, d) = _compare(monkeypatch, device, ch, leaves, cost, tau, dts)
    _env(monkeypatch, True)
    eager = _call(eng, lv, c, tau, d)
    n0 = lib().trex_debug_fused4_launches()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        f, dc, _, _ = eng.fwd_bwd(lv, c, tau, d)
    assert lib().trex_debug_fused4_launches() - n0 == 1
    out = dict(dp=f.dp, tree_score=f.tree_score, d_cost=dc)
    for rep in range(2):
        for v in out.values():
            v.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in eager:
            G.assert_bitwise(out[k], eager[k], f"{k}: replay {rep} vs eager")


def _fwd_bwd_prog(run, plan, prog, leaves, cost, L, tau, dts):
    """trex_sankoff_fwd_bwd_prog on guarded buffers (tests/_guard.py)"""
    st = stream_handle(run.device)
    pl, lv, c = run.input("plan", plan.host), run.input("leaves", leaves), run.input("cost", cost)
    pg = run.input("prog", prog)
    d = run.input("d_tree_score", dts)
    dp = run.output("dp", (plan.B, plan.n_int, L, Q), G.F32)
    ts = run.output("tree_score", (plan.B,), G.F32)
    dc = run.output("d_cost", (Q, Q), G.F32)
    nb = int(lib().trex_workspace_bytes(plan.B, L, plan.n_all, Q))
    ws = run.workspace(nb, init=True)
    check(lib().trex_sankoff_fwd_bwd_prog(ptr(pl), plan.slot_word, ptr(lv), ptr(c), plan.B, L,
                                          plan.n_all, Q, float(tau), 0, ptr(dp), None, ptr(ts),
                                          ptr(d), ptr(dc), None, None, ptr(ws), nb, st, ptr(pg)))


@pytest.mark.parametrize("shape", [lambda: shape_small(3), shape_32], ids=["3taxa", "32taxa"])
def test_h_guard_protocol(monkeypatch, device, shape):
    """the loads issued for steps before record 0 and past the last record stay
    inside the program; nothing is written outside dp, tree_score, d_cost"""
    ch, leaves, cost, tau, dts = shape()
    _env(monkeypatch, True)
    plan = TreePlan(ch)
    L = leaves.shape[2]
    eng = SankoffEngine(plan, L, Q, device)
    prog = eng.fused4_prog.cpu().numpy()
    lv, c, d = _dev(leaves, device), _dev(cost, device), _dev(dts, device)
    n0 = lib().trex_debug_fused4_launches()

    def r0():
        f, dc, _, _ = eng.fwd_bwd(lv, c, tau, d)
        return dict(dp=f.dp, tree_score=f.tree_score, d_cost=dc)

    G.protocol(device, r0, lambda run: _fwd_bwd_prog(run, plan, prog, leaves, cost, L, tau, dts))
    assert lib().trex_debug_fused4_launches() - n0 == 3
