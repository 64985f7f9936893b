"""The fused Q = 4 softmin kernel on the predecoded program
(sankoff_fused4.hip) against the generic fused kernel, bit for bit.

Every case runs the one-wave kernels (TREX_WIDE_SMALLQ=0) and compares the call
with TREX_FUSED4 unset (the new kernel, checked by its launch counter) against
TREX_FUSED4=0 (sankoff_kernel<4, true, 3>): dp, tree_score and d_cost hold the
same bytes.  No oracle and no tolerance here: the values are pinned by the
parity files, which run the default path.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import _guard as G
from _cases import (balanced_children, general_cost, hamming, random_leaves, random_topologies,
                    weird_children)
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


def _dev(x, device):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to(device).contiguous()


def shape_a():
    """2 tiles, the second with 4 live lanes; 6 items for 8 XCD shares"""
    return (random_topologies(3, 13, seed=11), random_leaves(3, 13, 68, Q, seed=12), hamming(Q),
            0.5, None)


def shape_b():
    """asymmetric cost with a non-zero diagonal: the non-SYM body"""
    rng = np.random.default_rng(21)
    return (random_topologies(9, 32, seed=22), random_leaves(9, 32, 200, Q, seed=23, missing=0.1),
            general_cost(Q, 24, "asym_frac"), 0.7, rng.uniform(0.5, 2.0, 9).astype(np.float32))


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


def _compare(monkeypatch, device, ch, leaves, cost, tau, dts, *, takes=True):
    _env(monkeypatch, True)
    eng = SankoffEngine(TreePlan(ch), leaves.shape[2], Q, device)
    assert (eng.fused4_prog is not None) == takes
    lv, c, d = _dev(leaves, device), _dev(cost, device), _dev(dts, device)
    n0 = lib().trex_debug_fused4_launches()
    new = _call(eng, lv, c, tau, d)
    assert lib().trex_debug_fused4_launches() - n0 == (1 if takes else 0)
    _env(monkeypatch, False)
    old = _call(eng, lv, c, tau, d)
    assert lib().trex_debug_fused4_launches() - n0 == (1 if takes else 0)
    for k in old:
        G.assert_bitwise(new[k], old[k], f"{k}: TREX_FUSED4 unset vs 0")
    assert torch.isfinite(new["d_cost"]).all() and new["d_cost"].abs().sum() > 0
    return eng, (lv, c, d)


def test_a_two_tiles_symmetric(monkeypatch, device):
    _compare(monkeypatch, device, *shape_a())


def test_b_asymmetric_missing_codes_weighted(monkeypatch, device):
    _compare(monkeypatch, device, *shape_b())


@pytest.mark.parametrize("tree", ["balanced", "pectinate"])
def test_c_balanced_and_pectinate(monkeypatch, device, tree):
    ch = balanced_children(16, B=2) if tree == "balanced" else pectinate(16)
    leaves = random_leaves(ch.shape[0], 16, 64, Q, seed=31)
    _compare(monkeypatch, device, ch, leaves, hamming(Q), 0.5, None)


def test_d_general_leaf_tables(monkeypatch, device):
    """tau = 5000: exp(-(1e5 - 1) / tau) is no underflow, the leaf tables hold
    the general message / weights of the 1e5 rows"""
    ch, leaves, cost, _, _ = shape_a()
    _compare(monkeypatch, device, ch, leaves, cost, 5000.0, None)


def test_e_non_factored_branch(monkeypatch, device):
    """range(C) / tau > 40: the launch runs the per-row stabilised softmin"""
    ch, leaves, _, _, _ = shape_a()
    cost = general_cost(Q, 41, "asym_wide")
    tau = 0.05
    assert (cost.max() - cost.min()) / tau > 40
    _compare(monkeypatch, device, ch, leaves, cost, tau, None)


@pytest.mark.parametrize("case", ["fwdref", "dag"])
def test_f_refused_plan_runs_the_generic_kernel(monkeypatch, device, case):
    ch = weird_children(case)[None]
    leaves = random_leaves(1, 8, 68, Q, seed=51)
    _compare(monkeypatch, device, ch, leaves, hamming(Q), 0.5, None, takes=False)


def test_g_captured_replay(monkeypatch, device):
    ch, leaves, cost, tau, dts = shape_a()
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
    """trex_sankoff_fwd_bwd_prog on guarded buffers (tests/_guard.py); no site
    scores, marginals or ancestral states: they are outside the kernel's scope"""
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


@pytest.mark.parametrize("shape", [shape_a, shape_b], ids=["a", "b"])
def test_h_guard_protocol(monkeypatch, device, shape):
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
