"""CPU tests of the NNI host side: the planner's move table, apply_nni, the
refusals.  No kernel is launched here."""

from __future__ import annotations

import numpy as np
import pytest

import _nni_ref as R
from _cases import balanced_children, random_topologies, weird_children
from trex_amd import TreePlan, TrexError, apply_nni
from trex_amd._lib import TREX_E_ARG, TREX_E_TOPOLOGY, TREX_PLAN_HEADER_INTS


def _trees(n):
    out = [random_topologies(8, n, seed=100 + n)]
    if n & (n - 1) == 0 and n >= 4:
        out.append(balanced_children(n))
    return out


@pytest.mark.parametrize("n", [3, 4, 9, 32])
def test_nni_table_matches_python_derivation(n):
    for ch in _trees(n):
        plan = TreePlan(ch)
        tab = plan.nni_table
        assert tab.dtype == np.int32 and tab.shape == (ch.shape[0], n - 2, 4)
        for b in range(ch.shape[0]):
            np.testing.assert_array_equal(tab[b], R.nni_table_ref(ch[b]))


@pytest.mark.parametrize("n", [3, 4, 9, 32])
def test_nni_plan_preorder_entries(n):
    """Every internal row once, the root first, a parent before its child,
    the sibling descriptor naming the other child of that parent."""
    for ch in _trees(n):
        plan = TreePlan(ch)
        ni, nl = plan.n_int, plan.n_leaves
        body = plan.nni_host[TREX_PLAN_HEADER_INTS:].reshape(plan.B, 8 * ni - 4)
        for b in range(plan.B):
            pre = body[b, :4 * ni].reshape(ni, 4)
            parent, sibling = R.relatives(ch[b])
            assert sorted(pre[:, 0]) == list(range(ni))
            assert tuple(pre[0, :2]) == (ni - 1, -1)
            seen = set()
            for row, prow, sd, _ in pre:
                if prow >= 0:
                    assert prow in seen
                    assert prow + nl == parent[row + nl]
                    s = (sd & 0xFFFF) + (nl if (sd >> 24) == 2 else 0)
                    assert (sd >> 24) in (1, 2) and s == sibling[row + nl]
                seen.add(row)


@pytest.mark.parametrize("n", [3, 4, 9, 32])
def test_apply_nni_is_valid_and_is_the_hand_swapped_tree(n):
    for ch in _trees(n):
        for b in range(min(3, ch.shape[0])):
            n_all = ch.shape[1]
            nl = (n_all + 1) // 2
            fam0 = R.leaf_sets(ch[b])
            for v in range(nl, n_all - 1):
                for k in (0, 1):
                    nb = apply_nni(ch[b], v, k)
                    assert nb.dtype == np.int32 and nb.shape == (n_all, 2)
                    assert (nb[:nl] == -1).all()  # leaf rows unused, as random_topologies
                    for node in range(nl, n_all):
                        assert 0 <= nb[node, 0] < nb[node, 1] < node
                    assert sorted(nb[nl:].reshape(-1)) == list(range(n_all - 1))
                    np.testing.assert_array_equal(nb, R.apply_nni_ref(ch[b], v, k))
                    fam = R.leaf_sets(nb)
                    assert fam == R.leaf_sets(R.hand_swap(ch[b], v, k))
                    assert fam != fam0  # a neighbour is a different tree
                    assert len(fam ^ fam0) == 2  # exactly one clade replaced
                    TreePlan(nb).nni_table  # accepted by both planners
                    # the inverse move restores the original leaf-set family
                    back = [(v2, k2) for v2 in range(nl, n_all - 1) for k2 in (0, 1)
                            if R.leaf_sets(apply_nni(nb, v2, k2)) == fam0]
                    assert len(back) >= 1


def test_distinct_neighbours_of_a_tree_differ():
    ch = random_topologies(1, 9, seed=5)[0]
    fams = [frozenset(R.leaf_sets(apply_nni(ch, v, k))) for v in range(9, 16) for k in (0, 1)]
    assert len(set(fams)) == len(fams) == 14


@pytest.mark.parametrize("case", ["fwdref", "dag", "cycle"])
def test_weird_children_are_refused(case):
    plan = TreePlan(weird_children(case))  # the forward planner takes them
    with pytest.raises(TrexError) as e:
        plan.nni_table
    assert e.value.code in (TREX_E_TOPOLOGY, TREX_E_ARG)


def test_other_improper_trees_are_refused():
    good = random_topologies(1, 6, seed=1)[0]
    bad = []
    c = good.copy(); c[7, 1] = -1; bad.append(c)  # -1 fill
    c = good.copy(); c[8] = (c[8, 0], c[8, 0]); bad.append(c)  # the same child twice
    c = good.copy(); c[9, 0] = c[8, 0]; bad.append(c)  # two parents (and an orphan)
    c = good.copy(); c[6, 0] = 6; bad.append(c)  # self reference
    for c in bad:
        with pytest.raises(TrexError) as e:
            TreePlan(c).nni_table
        assert e.value.code == TREX_E_TOPOLOGY
    # a batch is refused when any of its trees is
    with pytest.raises(TrexError):
        TreePlan(np.stack([good, bad[0]])).nni_table
    assert TreePlan(np.stack([good, good])).nni_table.shape == (2, 4, 4)


def test_two_leaves_are_refused():
    ch = np.array([[-1, -1], [-1, -1], [0, 1]], dtype=np.int32)
    plan = TreePlan(ch)
    with pytest.raises(TrexError) as e:
        plan.nni_table
    assert e.value.code in (TREX_E_TOPOLOGY, TREX_E_ARG)


def test_apply_nni_rejects_bad_moves():
    ch = random_topologies(1, 5, seed=0)[0]
    for v, k in ((8, 0), (4, 0), (5, 2), (-1, 0)):  # root, leaf, bad k, bad id
        with pytest.raises(ValueError):
            apply_nni(ch, v, k)


def test_existing_plan_is_unchanged_by_the_nni_plan():
    ch = random_topologies(5, 9, seed=3)
    plan = TreePlan(ch)
    before = plan.host.copy()
    word = plan.slot_word
    plan.nni_table
    plan.nni_host
    assert np.array_equal(plan.host, before) and plan.host.tobytes() == before.tobytes()
    assert plan.slot_word == word
    assert np.array_equal(TreePlan(ch).host, before)
