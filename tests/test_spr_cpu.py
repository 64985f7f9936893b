"""CPU tests of the SPR host side: apply_spr, the SPR plan, the refusals, the
``moves`` argument.  No kernel is launched here."""

from __future__ import annotations

import numpy as np
import pytest

import _nni_ref as R
import _spr_ref as S
from _cases import balanced_children, random_topologies, weird_children
from trex_amd import (TreePlan, TrexError, apply_spr, bootstrap_search, parsimony_ratchet,
                      parsimony_search)
from trex_amd._lib import TREX_E_ARG, TREX_E_TOPOLOGY, TREX_PLAN_HEADER_INTS, lib


def caterpillar(n):
    ch = np.full((2 * n - 1, 2), -1, dtype=np.int32)
    ch[n] = (0, 1)
    for k in range(1, n - 1):
        ch[n + k] = (k + 1, n + k - 1)
    return ch


def _trees():
    out = [caterpillar(7), balanced_children(8)[0]]
    for n in (3, 4, 6, 9):
        out.extend(random_topologies(2, n, seed=500 + n))
    return out


def test_apply_spr_on_every_move():
    for ch in _trees():
        n_all = ch.shape[0]
        n = (n_all + 1) // 2
        ok = S.valid_mask(ch)
        parent, sibling = R.relatives(ch)
        fam0 = R.leaf_sets(ch)
        clade = [frozenset(y for y in S.subtree(ch, x) if y < n) for x in range(n_all)]
        for v in range(n_all - 1):
            inside_v = S.subtree(ch, v)
            below_v = clade[v]
            u = parent[v]
            for x in range(n_all):
                if not ok[v, x]:
                    with pytest.raises(ValueError):
                        apply_spr(ch, v, x)
                    continue
                g = apply_spr(ch, v, x)
                assert g.dtype == np.int32 and g.shape == (n_all, 2) and (g[:n] == -1).all()
                for node in range(n, n_all):
                    assert 0 <= g[node, 0] < g[node, 1] < node
                np.testing.assert_array_equal(g, S.apply_spr_ref(ch, v, x))
                TreePlan(g).spr_host  # a proper tree again
                # T's clades with v moved: u's clade goes, v's other ancestors
                # lose v's leaves, x's proper ancestors (u apart) gain them,
                # and x's leaves with v's are the one new clade
                want = {clade[x] | below_v}
                for y in range(n, n_all):
                    if y == u:
                        continue
                    c = clade[y]
                    if y not in inside_v:
                        c = c - below_v
                        if clade[x] < clade[y]:
                            c = c | below_v
                    want.add(c)
                assert R.leaf_sets(g) == want, (v, x)
                if x == sibling[v]:
                    assert R.leaf_sets(g) == fam0  # the tree itself


def test_apply_spr_rejects_bad_input():
    ch = random_topologies(1, 5, seed=0)[0]
    for v, x in ((8, 0), (-1, 0), (9, 0), (0, -1), (0, 9), (0, 100)):
        with pytest.raises(ValueError):
            apply_spr(ch, v, x)
    with pytest.raises(ValueError):
        apply_spr(ch[:8], 0, 1)
    for case in ("fwdref", "dag", "cycle"):
        with pytest.raises(ValueError):
            apply_spr(weird_children(case), 0, 1)


def _plan_ref(ch):
    """The SPR plan's region of one tree, restated: node records {parent,
    sibling, entry, exit} of a pre-order DFS over all nodes (children in stored
    order), then the internal nodes by ascending entry {row, c0, c1, 0}."""
    n_all = ch.shape[0]
    nl = (n_all + 1) // 2
    parent, sibling = R.relatives(ch)
    node = np.zeros((n_all, 4), dtype=np.int32)
    walk = []
    clock = [0]

    def rec(x):
        node[x, 0] = parent.get(x, -1)
        node[x, 1] = sibling.get(x, -1)
        node[x, 2] = clock[0]
        clock[0] += 1
        if x >= nl:
            walk.append([x - nl, int(ch[x, 0]), int(ch[x, 1]), 0])
            rec(int(ch[x, 0]))
            rec(int(ch[x, 1]))
        node[x, 3] = clock[0]

    rec(n_all - 1)
    return np.concatenate([node.reshape(-1), np.array(walk, dtype=np.int32).reshape(-1)])


@pytest.mark.parametrize("n", range(3, 10))
def test_spr_plan_matches_python_derivation(n):
    ch = random_topologies(4, n, seed=200 + n)
    if n == 7:
        ch[1] = caterpillar(7)
    plan = TreePlan(ch)
    nl, ni, n_all = plan.n_leaves, plan.n_int, plan.n_all
    host = plan.spr_host
    per = 4 * n_all + 4 * ni
    assert lib().trex_spr_plan_ints(4, n_all) == TREX_PLAN_HEADER_INTS + 4 * per
    assert host.dtype == np.int32 and host.shape == (TREX_PLAN_HEADER_INTS + 4 * per,)
    assert tuple(host[1:5]) == (4, n_all, nl, ni) and not host[5:TREX_PLAN_HEADER_INTS].any()
    body = host[TREX_PLAN_HEADER_INTS:].reshape(4, per)
    for b in range(4):
        np.testing.assert_array_equal(body[b], _plan_ref(ch[b]))
        node = body[b, :4 * n_all].reshape(n_all, 4)
        # the interval test is the subtree test
        for v in range(n_all):
            inside = {x for x in range(n_all) if node[v, 2] <= node[x, 2] < node[v, 3]}
            assert inside == S.subtree(ch[b], v)
    assert plan.spr_host is host  # built once


@pytest.mark.parametrize("case", ["fwdref", "dag", "cycle"])
def test_weird_children_are_refused(case):
    plan = TreePlan(weird_children(case))  # the forward planner takes them
    with pytest.raises(TrexError) as e:
        plan.spr_host
    with pytest.raises(TrexError) as e_nni:
        plan.nni_host
    assert e.value.code == e_nni.value.code
    assert e.value.code in (TREX_E_TOPOLOGY, TREX_E_ARG)


def test_spr_builder_refuses_what_the_nni_builder_refuses():
    good = random_topologies(1, 6, seed=1)[0]
    bad = []
    c = good.copy(); c[7, 1] = -1; bad.append(c)  # -1 fill
    c = good.copy(); c[8] = (c[8, 0], c[8, 0]); bad.append(c)  # the same child twice
    c = good.copy(); c[9, 0] = c[8, 0]; bad.append(c)  # two parents (and an orphan)
    c = good.copy(); c[6, 0] = 6; bad.append(c)  # self reference
    two = np.array([[-1, -1], [-1, -1], [0, 1]], dtype=np.int32)
    for c in bad + [np.stack([good, bad[0]]), two]:
        with pytest.raises(TrexError) as e:
            TreePlan(c).spr_host
        with pytest.raises(TrexError) as e_nni:
            TreePlan(c).nni_host
        assert e.value.code == e_nni.value.code
        if c.ndim == 2 and c.shape[0] > 3:
            assert e.value.code == TREX_E_TOPOLOGY
            with pytest.raises(ValueError):
                apply_spr(c, 0, 1)
    TreePlan(good).spr_host
    # the C entry points on the raw arguments: same codes
    L = lib()
    ch = np.ascontiguousarray(good[None])
    buf = np.zeros(max(L.trex_spr_plan_ints(1, 11), L.trex_nni_plan_ints(1, 11)), dtype=np.int32)
    for args in ((None, 1, 11, buf.ctypes.data), (ch.ctypes.data, 1, 11, None),
                 (ch.ctypes.data, 0, 11, buf.ctypes.data), (ch.ctypes.data, 1, 10, buf.ctypes.data),
                 (ch.ctypes.data, 1, 3, buf.ctypes.data)):
        rc = L.trex_spr_plan_build(*args)
        assert rc == L.trex_nni_plan_build(*args) and rc < 0
    assert L.trex_spr_plan_ints(0, 11) == 0 and L.trex_spr_plan_ints(1, 2) == 0


def test_other_plans_are_unchanged_by_the_spr_plan():
    ch = random_topologies(5, 9, seed=3)
    plan = TreePlan(ch)
    before, word = plan.host.copy(), plan.slot_word
    nni_before, attach_before = plan.nni_host.copy(), plan.attach_host.copy()
    plan.spr_host
    assert plan.host.tobytes() == before.tobytes() and plan.slot_word == word
    assert plan.nni_host.tobytes() == nni_before.tobytes()
    assert plan.attach_host.tobytes() == attach_before.tobytes()
    fresh = TreePlan(ch)
    assert fresh.host.tobytes() == before.tobytes()
    assert fresh.nni_host.tobytes() == nni_before.tobytes()
    assert fresh.attach_host.tobytes() == attach_before.tobytes()


def test_workspace_bytes_formula_and_overflow():
    L = lib()
    B, sites, n_all, Q = 3, 130, 11, 5
    tiles, ni = 3, 5
    part = (B * tiles * (n_all - 1) * n_all * 8 + 255) // 256 * 256
    assert L.trex_spr_workspace_bytes(B, sites, n_all, Q) == part + B * tiles * ni * 64 * Q * 4 + 256
    for bad in ((0, 8, 11, 4), (1, 0, 11, 4), (1, 8, 3, 4), (1, 8, 10, 4), (1, 8, 11, 1),
                (1, 8, 11, 21)):
        assert L.trex_spr_workspace_bytes(*bad) == 0
    # sizes that do not fit: refused, never wrapped
    assert L.trex_spr_workspace_bytes(1, 8, 65535, 4) == 0  # (n_all - 1) n_all > INT_MAX
    assert L.trex_spr_workspace_bytes(2 ** 31 - 1, 2 ** 31 - 1, 46339, 20) == 0
    big = L.trex_spr_workspace_bytes(1, 8, 46339, 4)
    assert big == (46338 * 46339 * 8 + 255) // 256 * 256 + 23169 * 64 * 4 * 4 + 256


def test_unknown_moves_are_rejected():
    """``moves`` is checked before anything touches the device."""
    lv = np.zeros((5, 7), dtype=np.int8)
    cost = np.ones((4, 4), dtype=np.float32) - np.eye(4, dtype=np.float32)
    ch = random_topologies(1, 5, seed=0)
    for moves in ("x", "tbr", "", None, "SPR"):
        with pytest.raises(ValueError):
            parsimony_search(lv, cost, n_trees=1, moves=moves, device="cpu")
        with pytest.raises(ValueError):
            parsimony_ratchet(ch, lv, cost, moves=moves, device="cpu")
        with pytest.raises(ValueError):
            bootstrap_search(lv, cost, n_replicates=2, moves=moves, device="cpu")
