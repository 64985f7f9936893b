"""Pair tables of the Q <= 4 lane-per-site kernel (sankoff.hip,
TREX_PAIR_TABLES): a deferred cherry's message to its parent (every mode) and
the u / 1 / s of its parent edge's adjoint (factored softmin) are looked up by
the cherry's two leaf codes instead of being computed per site.  A lookup is
bitwise what the lanes compute, so every check against the computing path
(`TREX_DEFER=0` plans) is bitwise; the fp64 oracle bounds are the suite's own
(tests/_cases.py).
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from _cases import (assert_dp_close, assert_grad_close, balanced_children, cond_rtol, general_cost,
                    int_cost, random_leaves, random_topologies, weird_children)
from oracle.softmin_ref import batched_fwd_bwd_ref
from trex_amd import SankoffEngine, TreePlan
from trex_amd.ragged import RaggedSankoffEngine, RaggedTreePlan

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def lane_per_site(monkeypatch):
    """sankoff_kernel (one lane per site) takes every call of this file."""
    monkeypatch.setenv("TREX_WIDE_SMALLQ", "0")


def _dev(x, device, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(device).contiguous()


def _kinds(ch):
    """Per internal row: its two children as ("leaf", i) / ("int", r) / ("sent", -1)
    (trex's rule: -1 and forward references are 1e5 rows)."""
    n_all = ch.shape[0]
    nl = (n_all + 1) // 2
    out = []
    for node in range(nl, n_all):
        pair = []
        for c in (int(x) for x in ch[node]):
            if c == -1 or c >= node:
                pair.append(("sent", -1))
            elif c < nl:
                pair.append(("leaf", c))
            else:
                pair.append(("int", c - nl))
        out.append(pair)
    return out


def _reached(ch):
    """Internal rows the adjoint reaches from the root (the others' marginals
    and states are not written)."""
    kinds = _kinds(ch)
    reach = np.zeros(len(kinds), dtype=bool)
    reach[-1] = True
    for r in range(len(kinds) - 1, -1, -1):
        if reach[r]:
            for kind, idx in kinds[r]:
                if kind == "int":
                    reach[idx] = True
    return reach


def _pair_leaves(ch, L, Q, seed):
    """(1, n_leaves, L) codes: random with 10 % missing, except the leaves of
    every cherry (no internal child): at site s its first child has code
    s % (Q + 1), its second (s // (Q + 1)) % (Q + 1), code Q written as -1 on
    even sites and 127 on odd ones (both are the all-1e5 row) -- every ordered
    pair of the (Q + 1)^2 within the first (Q + 1)^2 sites, in both tiles'
    worth of lanes."""
    nl = (ch.shape[0] + 1) // 2
    leaves = random_leaves(1, nl, L, Q, seed=seed, missing=0.1)
    s = np.arange(L)
    miss = np.where(s % 2 == 0, -1, 127)
    codes = [s % (Q + 1), (s // (Q + 1)) % (Q + 1)]
    n_cherries = 0
    for pair in _kinds(ch):
        if any(kind == "int" for kind, _ in pair):
            continue
        n_cherries += 1
        for k, (kind, idx) in enumerate(pair):
            if kind == "leaf":
                leaves[0, idx] = np.where(codes[k] == Q, miss, codes[k]).astype(np.int8)
    assert n_cherries >= 2
    return leaves


def _tree(name):
    if name == "balanced":
        return balanced_children(8)[0]  # four deferred cherries
    return weird_children(name)


# tau, cost ceiling, what it exercises
MODES = {
    "hard": (0.0, 4),
    "factored": (0.5, 4),
    "direct": (0.05, 9),    # range(C) / tau > 40: the per-row stabilised softmin
    "general": (4000.0, 4),  # exp(-1e5 / tau) is not negligible: general leaf tables
}
COST_SEED = 4  # with hi = 9 its range is 9 at every Q: tau = 0.05 takes the direct path


def _run_all(eng, lv, c, tau, dts):
    f, dc, mg, an = eng.fwd_bwd(lv, c, tau, dts, site_score=True, marginals=True, anc_states=True)
    return f, dc, mg, an


def _cost(Q, mode, cost_kind):
    """"sym": the symmetric zero-diagonal integer matrix; "asym_int": every
    entry on its own, diagonal 1..2 (a cherry of two equal codes i under
    state i costs 2 C[i][i] != 0; C[i][a] and C[a][i] differ), with the wide
    range ("asym_wide") for the direct mode.  The every-ordered-code-pair
    leaf layout is what tells C[i][a] from C[a][i] in the tables; the sites
    with missing codes put 1e5 offsets into the tree score, so the score
    condition of assert_cost_is_general is not asked of these inputs."""
    if cost_kind == "sym":
        return int_cost(Q, seed=COST_SEED, hi=MODES[mode][1])
    cost = general_cost(Q, 1, "asym_wide" if mode == "direct" else "asym_int")
    assert (cost != cost.T).any() and (np.diag(cost) != 0).all() and cost.min() != 0
    return cost


# the symmetric cases keep their ids; "-asym_int" marks the new ones
MODE_KINDS = ([pytest.param(m, "sym", id=m) for m in MODES]
              + [pytest.param(m, "asym_int", id=f"{m}-asym_int") for m in MODES])


@pytest.mark.parametrize("mode,cost_kind", MODE_KINDS)
@pytest.mark.parametrize("tree", ["balanced", "fwdref", "dag"])
@pytest.mark.parametrize("Q", [2, 3, 4])
def test_every_code_pair_every_mode(device, monkeypatch, Q, tree, mode, cost_kind):
    """Every ordered pair of leaf codes (missing included, as -1 and as 127)
    under a cherry, in the hard, factored, direct and general-leaf-table
    modes, on trees with four deferred cherries ("balanced"), with a cherry
    holding a -1 child and one holding a forward-referenced 1e5 row
    ("fwdref"), and with a two-parent cherry that must keep the computing
    path ("dag").  L = 70: two tiles, the second with 6 active lanes.

    The fused launch equals forward + backward bitwise; the table path equals
    the computing path (TREX_DEFER=0 plan) bitwise on DP, scores, marginals
    and states (dC: summation order only); DP, tree score and dC meet the
    fp64 oracle's bounds, tau = 4 000 included (the parent commit passes the
    same comparison)."""
    tau, _ = MODES[mode]
    L = 70
    ch = _tree(tree)
    leaves = _pair_leaves(ch, L, Q, seed=10 * Q + 1)
    cost = _cost(Q, mode, cost_kind)
    if mode == "direct":
        assert (cost.max() - cost.min()) / tau > 40.0
    seen = set()
    for pair in _kinds(ch):
        if all(kind == "leaf" for kind, _ in pair):
            a, b = (np.where((leaves[0, idx] < 0) | (leaves[0, idx] >= Q), Q, leaves[0, idx])
                    for _, idx in pair)
            seen |= set(zip(a.tolist(), b.tolist()))
    assert len(seen) == (Q + 1) ** 2
    lv = _dev(leaves, device)
    c = _dev(cost, device, torch.float32)
    dts = torch.tensor([1.5], device=device)
    reach = torch.as_tensor(_reached(ch), device=device)

    monkeypatch.delenv("TREX_DEFER", raising=False)
    plan = TreePlan(ch[None])
    n_deferred = int(((plan.fwd_steps[0][:, 3] & 8) != 0).sum())
    assert n_deferred == {"balanced": 4, "fwdref": 4, "dag": 2}[tree]
    eng = SankoffEngine(plan, L, Q, device)
    f, dc, mg, an = _run_all(eng, lv, c, tau, dts)

    # fused == forward + backward
    f1 = eng.forward(lv, c, tau, site_score=True)
    dc1, mg1, an1 = eng.backward(lv, c, tau, f1.dp, dts, marginals=True, anc_states=True)
    assert torch.equal(f1.dp, f.dp)
    assert torch.equal(f1.tree_score, f.tree_score) and torch.equal(f1.site_score, f.site_score)
    assert torch.equal(dc1, dc)
    assert torch.equal(mg1[:, reach], mg[:, reach]) and torch.equal(an1[:, reach], an[:, reach])

    # table path == computing path
    monkeypatch.setenv("TREX_DEFER", "0")
    plan0 = TreePlan(ch[None])
    assert not ((plan0.fwd_steps[0][:, 3] & 8) != 0).any()
    eng0 = SankoffEngine(plan0, L, Q, device)
    f0, dc0, mg0, an0 = _run_all(eng0, lv, c, tau, dts)
    assert torch.equal(f0.dp, f.dp)
    assert torch.equal(f0.tree_score, f.tree_score) and torch.equal(f0.site_score, f.site_score)
    assert torch.equal(mg0[:, reach], mg[:, reach]) and torch.equal(an0[:, reach], an[:, reach])
    np.testing.assert_allclose(dc.cpu().numpy(), dc0.cpu().numpy(), rtol=1e-5, atol=1e-3)

    # fp64 oracle
    ref = batched_fwd_bwd_ref(ch[None], leaves, cost, tau, d_tree_score=dts.cpu().numpy())
    got_dp = eng.state_rows(f.dp).cpu().numpy()
    if tau == 0.0:
        np.testing.assert_array_equal(got_dp, ref["dp"].astype(np.float32))
        np.testing.assert_allclose(f.tree_score.cpu().numpy(), ref["tree_score"], rtol=1e-5)
        np.testing.assert_allclose(dc.cpu().numpy(), ref["d_cost"], rtol=1e-6)
    else:
        assert_dp_close(got_dp, ref)
        np.testing.assert_allclose(f.tree_score.cpu().numpy(), ref["tree_score"], rtol=1e-5)
        assert_grad_close(dc.cpu().numpy(), ref["d_cost"], rtol=cond_rtol(ref["dp"], tau))


def _oracle_check(ch, leaves, cost, tau, eng, f, dc):
    ref = batched_fwd_bwd_ref(ch, leaves, cost, tau)
    assert_dp_close(eng.state_rows(f.dp).cpu().numpy(), ref)
    np.testing.assert_allclose(f.tree_score.cpu().numpy(), ref["tree_score"], rtol=1e-5)
    assert_grad_close(dc.cpu().numpy(), ref["d_cost"], rtol=cond_rtol(ref["dp"], tau))


@pytest.mark.parametrize("case", ["deep-stack", "byte-leaf-path"])
def test_lds_map_after_the_tables(device, case):
    """The slot stack and the leaf tile lie behind the tables: the deepest
    stack of a 64-leaf tree (balanced, L = 70), and trees of more than 64
    leaves at L & 3 != 0 (80 leaves, L = 66: the byte-per-lane leaf path
    fills the tile), factored softmin at Q = 4, against the fp64 oracle."""
    Q, tau = 4, 0.5
    if case == "deep-stack":
        ch, L = balanced_children(64), 70
    else:
        ch, L = random_topologies(2, 80, seed=5), 66
    nl = (ch.shape[1] + 1) // 2
    leaves = random_leaves(ch.shape[0], nl, L, Q, seed=6, missing=0.1)
    cost = int_cost(Q, seed=7, hi=4)
    eng = SankoffEngine(TreePlan(ch), L, Q, device)
    f, dc, _, _ = eng.fwd_bwd(_dev(leaves, device), _dev(cost, device, torch.float32), tau)
    _oracle_check(ch, leaves, cost, tau, eng, f, dc)


def test_ragged_body_matches_uniform(device):
    """The ragged launch shares the body: two balanced 64-leaf trees with
    different site counts in one ragged batch give, per tree, bitwise the DP
    table and tree score of the uniform engine."""
    Q, tau = 4, 0.5
    ch = balanced_children(64)[0]
    Ls = [70, 130]
    cost = int_cost(Q, seed=7, hi=4)
    c = _dev(cost, device, torch.float32)
    leaves = [random_leaves(1, 64, L, Q, seed=8 + L, missing=0.1)[0] for L in Ls]
    rplan = RaggedTreePlan([ch, ch], Ls)
    reng = RaggedSankoffEngine(rplan, Q, device)
    ts, dp, _, _, _, _ = reng.fwd_bwd(_dev(rplan.pack_leaves(leaves), device), c, tau)
    for b, L in enumerate(Ls):
        eng = SankoffEngine(TreePlan(ch[None]), L, Q, device)
        f, _, _, _ = eng.fwd_bwd(_dev(leaves[b][None], device), c, tau)
        assert torch.equal(rplan.tree_rows(dp, b), f.dp[0])
        assert torch.equal(ts[b], f.tree_score[0])
