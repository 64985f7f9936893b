"""The fused Q = 4 kernel's 4-wave workgroups (sankoff_fused4.hip: one copy of
the leaf and pair tables per workgroup, a slot stack and leaf tile per wave)
against the generic one-wave fused kernel, bit for bit.

As in test_fused4_gpu.py every case runs under TREX_WIDE_SMALLQ=0 and compares
the call with TREX_FUSED4 unset (the fused4 kernel, checked by its launch
counter) against TREX_FUSED4=0 (sankoff_kernel<4, true, 3>): dp, tree_score
and d_cost hold the same bytes.  The shapes are the smallest that reach each
path of the workgroup: fewer items than a workgroup has waves, workgroups
whose last waves have no item, fewer workgroups than XCD shares, a second tile
with 4 live lanes, missing codes, plans without deferral, a deep slot stack
with the largest leaf tile, the direct-softmin branch (the generic body per
wave) from a short workgroup, general leaf tables, graph replay, and the
guard-band protocol.
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


def two_pitchforks():
    """6 leaves: 7 = (leaf 2, cherry 6), 9 = (cherry 8, leaf 5), root 10 = (7, 9)"""
    ch = np.full((11, 2), -1, dtype=np.int32)
    ch[6], ch[7], ch[8], ch[9], ch[10] = (0, 1), (2, 6), (3, 4), (8, 5), (7, 9)
    return ch[None]


def shape_13():
    """5 trees x 6 tiles = 30 items: 8 workgroups, the last with two waves
    idle; every table position sees a missing code; the non-SYM body"""
    rng = np.random.default_rng(61)
    return (random_topologies(5, 13, seed=62), random_leaves(5, 13, 324, Q, seed=63, missing=0.3),
            general_cost(Q, 64, "asym_frac"), 0.7, rng.uniform(0.5, 2.0, 5).astype(np.float32))


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
    return eng, (lv, c, d), old


def test_a_pectinate4_two_items_in_one_workgroup(monkeypatch, device):
    """the second tile has 4 live lanes; waves 2 and 3 have no item"""
    leaves = random_leaves(1, 4, 68, Q, seed=71, missing=0.2)
    _compare(monkeypatch, device, pectinate(4), leaves, hamming(Q), 0.5, None)


def test_b_pectinate3_two_steps(monkeypatch, device):
    leaves = random_leaves(1, 3, 68, Q, seed=72, missing=0.2)
    _compare(monkeypatch, device, pectinate(3), leaves, hamming(Q), 0.5, None)


def test_c_two_pitchforks_asymmetric(monkeypatch, device):
    leaves = random_leaves(1, 6, 68, Q, seed=73, missing=0.2)
    _compare(monkeypatch, device, two_pitchforks(), leaves, general_cost(Q, 74, "asym_frac"), 0.6,
             None)


def test_d_short_last_workgroup_missing_codes_weighted(monkeypatch, device):
    ch, leaves, cost, tau, dts = shape_13()
    _compare(monkeypatch, device, ch, leaves, cost, tau, dts)
    assert (leaves.shape[0] * ((leaves.shape[2] + 63) // 64)) % 4 == 2


def test_e_plans_without_deferral(monkeypatch, device):
    monkeypatch.setenv("TREX_DEFER", "0")
    rng = np.random.default_rng(81)
    ch = random_topologies(9, 32, seed=82)
    leaves = random_leaves(9, 32, 200, Q, seed=83, missing=0.1)
    _compare(monkeypatch, device, ch, leaves, general_cost(Q, 84, "asym_frac"), 0.7,
             rng.uniform(0.5, 2.0, 9).astype(np.float32))


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


def test_g_balanced64_deep_stack_large_lds(monkeypatch, device):
    ch = balanced_children(64, B=2)
    leaves = random_leaves(2, 64, 64, Q, seed=91, missing=0.1)
    _compare(monkeypatch, device, ch, leaves, hamming(Q), 0.5, None)


def test_h_direct_softmin_from_a_multi_wave_workgroup(monkeypatch, device):
    """range(C) / tau > 40: every wave runs the generic body on the shared
    tables and its own slot stack; the last workgroup is short"""
    ch, leaves, _, _, dts = shape_13()
    cost = general_cost(Q, 41, "asym_wide")
    tau = 0.05
    assert (cost.max() - cost.min()) / tau > 40
    _compare(monkeypatch, device, ch, leaves, cost, tau, dts)


def test_i_general_leaf_tables(monkeypatch, device):
    """tau = 5000: the leaf tables hold the general message / weights of the
    1e5 rows, and the pair tables are built on them"""
    ch, leaves, cost, _, dts = shape_13()
    _compare(monkeypatch, device, ch, leaves, cost, 5000.0, dts)


def test_j_captured_replay(monkeypatch, device):
    ch, leaves, cost, tau, dts = shape_13()
    eng, (lv, c, d), _ = _compare(monkeypatch, device, ch, leaves, cost, tau, dts)
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


def test_k_guard_protocol(monkeypatch, device):
    ch, leaves, cost, tau, dts = shape_13()
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
