"""fp64 numpy references for the attachment scores and stepwise addition
(test side only; shares no code with trex_amd).

Two independent routes to the score of a tree after a subtree is attached on
the edge above node x:

* ``attach_ref``: the definitions -- inside and outside rows (``_nni_ref``),
  then the O(Q^2) evaluation per site and edge;
* ``brute_force`` / ``graft_ref``: the grown tree's child lists rebuilt
  explicitly (``insert_leaf_ref``, or a whole subtree joined by hand), then
  the fp64 oracle's tree score (oracle.softmin_ref.sankoff_fwd_bwd_ref).

``_self_check`` asserts once, at import, that the two agree.
"""

from __future__ import annotations

import numpy as np

import _nni_ref as R
from oracle.softmin_ref import sankoff_fwd_bwd_ref

SENT = R.SENT


def leaf_rows(codes, Q):
    """(L,) codes -> (L, Q) inside rows: 0 at the code, 1e5 elsewhere (-1: all 1e5)."""
    return np.where(np.asarray(codes)[:, None] == np.arange(Q)[None, :], 0.0, SENT)


def attach_ref(children, leaves, cost, tau, new_codes=None, sub_rows=None):
    """One tree.  (n_all,) tree scores after attaching the subtree with inside
    rows D_new (``new_codes`` (L,) or ``sub_rows`` (L, Q)) on the edge above
    every node x; x = n_all - 1 is a new root above the old one."""
    cost = np.asarray(cost, dtype=np.float64)
    Q = cost.shape[0]
    n_all = children.shape[0]
    nl = (n_all + 1) // 2
    r = R.nni_ref(children, leaves, cost, tau)
    D, O = r["inside"], r["outside"]  # (n_all, L, Q), (n_int, L, Q)
    Dn = leaf_rows(new_codes, Q) if sub_rows is None else np.asarray(sub_rows, dtype=np.float64)
    Mn = R._msg(cost, Dn, tau)
    M = [R._msg(cost, D[x], tau) for x in range(n_all)]
    parent, sibling = R.relatives(children)
    out = np.zeros(n_all)
    for x in range(n_all - 1):
        p, s = parent[x], sibling[x]
        Dw = M[x] + Mn
        out[x] = R.oplus(O[p - nl] + M[s] + R._msg(cost, Dw, tau), tau).sum()
    out[n_all - 1] = R.oplus(M[n_all - 1] + Mn, tau).sum()
    return out


def insert_leaf_ref(children, x):
    """Independent restatement of insert_leaf: new leaf n_leaves on the edge
    above x; internal nodes numbered in post-order by a recursive DFS that
    takes children in ascending id order (the new node in x's place), pairs
    stored ascending."""
    n_all = children.shape[0]
    nl = (n_all + 1) // 2
    out = np.full((n_all + 2, 2), -1, dtype=np.int32)
    counter = [nl + 1]

    def emit(a, b):
        me = counter[0]
        counter[0] += 1
        out[me] = (min(a, b), max(a, b))
        return me

    def rec(v):
        if v < nl:
            me = v
        else:
            lo, hi = sorted((int(children[v, 0]), int(children[v, 1])))
            n0 = rec(lo)
            n1 = rec(hi)
            me = emit(n0, n1)
        if v == x:
            me = emit(me, nl)  # the new leaf has no internal nodes: its turn emits nothing
        return me

    assert rec(n_all - 1) == n_all + 1
    return out


def relabel_ref(children, perm):
    """Leaf j renamed perm[j]; the DFS takes children in ascending order of
    their new leaf id / old internal id."""
    n_all = children.shape[0]
    nl = (n_all + 1) // 2
    out = np.full((n_all, 2), -1, dtype=np.int32)
    counter = [nl]

    def rec(v):
        if v < nl:
            return int(perm[v])
        kids = sorted((int(children[v, 0]), int(children[v, 1])),
                      key=lambda c: int(perm[c]) if c < nl else c)
        n0 = rec(kids[0])
        n1 = rec(kids[1])
        me = counter[0]
        counter[0] += 1
        out[me] = (min(n0, n1), max(n0, n1))
        return me

    assert rec(n_all - 1) == n_all - 1
    return out


def graft_ref(children_a, children_s, x):
    """Tree S joined by hand on the edge above node x of tree A: A's leaves
    keep their ids, S's leaf j is n_leaves(A) + j; any numbering with every
    child below its parent."""
    na = (children_a.shape[0] + 1) // 2
    ns = (children_s.shape[0] + 1) // 2
    n = na + ns
    out = np.full((2 * n - 1, 2), -1, dtype=np.int32)
    counter = [n]

    def emit(a, b):
        me = counter[0]
        counter[0] += 1
        out[me] = (min(a, b), max(a, b))
        return me

    def rec_s(v):
        if v < ns:
            return na + v
        return emit(rec_s(int(children_s[v, 0])), rec_s(int(children_s[v, 1])))

    def rec_a(v):
        me = v if v < na else emit(rec_a(int(children_a[v, 0])), rec_a(int(children_a[v, 1])))
        if v == x:
            me = emit(me, rec_s(children_s.shape[0] - 1))
        return me

    assert rec_a(children_a.shape[0] - 1) == 2 * n - 2
    return out


def brute_force(children, leaves_plus, cost, tau):
    """(n_all,) scores via rebuilt topologies + the oracle; leaves_plus
    (n_leaves + 1, L): the tree's leaves, then the new leaf."""
    n_all = children.shape[0]
    return np.array([sankoff_fwd_bwd_ref(insert_leaf_ref(children, x), leaves_plus, cost,
                                         tau)["tree_score"] for x in range(n_all)])


TRIPLETS = [np.array([[-1, -1]] * 3 + [[a, b], [c, 3]], dtype=np.int32)
            for a, b, c in ((0, 1, 2), (0, 2, 1), (1, 2, 0))]


def stepwise_ref(leaves, cost, order, tau):
    """The fp64 greedy for one addition sequence: the best of the three
    starting trees (ties: the lowest index), every further taxon on the edge
    of the first minimum (ties: the lowest node id).  Returns (children with
    the alignment's taxon ids, tree score)."""
    taxa = leaves[np.asarray(order)]
    start = [sankoff_fwd_bwd_ref(t, taxa[:3], cost, tau)["tree_score"] for t in TRIPLETS]
    ch = TRIPLETS[int(np.argmin(start))]
    for k in range(3, len(order)):
        sc = attach_ref(ch, taxa[:k], cost, tau, new_codes=taxa[k])
        ch = insert_leaf_ref(ch, int(np.argmin(sc)))
    ch = relabel_ref(ch, order)
    return ch, float(sankoff_fwd_bwd_ref(ch, leaves, cost, tau)["tree_score"])


def _self_check():
    from _cases import int_cost, random_leaves, random_topologies

    for n, Q, tau, seed in ((5, 3, 0.0, 1), (7, 4, 0.5, 2), (6, 5, 0.0, 3)):
        ch = random_topologies(1, n, seed=seed)[0]
        lv = random_leaves(1, n + 1, 9, Q, seed, missing=0.1 if tau == 0.0 else 0.0)[0]
        c = int_cost(Q, seed)
        if seed == 3:
            c = c + np.triu(np.ones_like(c), 1)  # asymmetric
        a = attach_ref(ch, lv[:n], c, tau, new_codes=lv[n])
        bf = brute_force(ch, lv, c, tau)
        # a whole subtree: its root's inside row, against the tree joined by hand
        chs = random_topologies(1, 3, seed=seed + 7)[0]
        lvs = random_leaves(1, 3, 9, Q, seed + 7)[0]
        rows = R.nni_ref(chs, lvs, c, tau)["inside"][-1]
        g = attach_ref(ch, lv[:n], c, tau, sub_rows=rows)
        both = np.concatenate([lv[:n], lvs])
        gf = np.array([sankoff_fwd_bwd_ref(graft_ref(ch, chs, x), both, c, tau)["tree_score"]
                       for x in range(2 * n - 1)])
        if tau == 0.0:
            assert np.array_equal(a, bf), (a, bf)
            assert np.array_equal(g, gf), (g, gf)
        else:
            np.testing.assert_allclose(a, bf, rtol=1e-12)
            np.testing.assert_allclose(g, gf, rtol=1e-12)


_self_check()
