"""fp64 numpy references for the NNI neighbour scores (test side only; shares
no code with trex_amd).

Two independent routes to the score of move (v, k) of a tree:

* ``nni_ref``: the definitions -- inside rows by a post-order pass, outside
  rows by a pre-order pass, the O(Q^2) move evaluation per site;
* ``brute_force``: the neighbour's child lists rebuilt explicitly
  (``apply_nni_ref``), then the fp64 oracle's tree score
  (oracle.softmin_ref.sankoff_fwd_bwd_ref).

``_self_check`` asserts once, at import, that the two agree.
"""

from __future__ import annotations

import numpy as np

from oracle.softmin_ref import sankoff_fwd_bwd_ref

SENT = 1e5


def oplus(x, tau, axis=-1):
    """min (tau = 0) or smin_tau over an axis, stabilised."""
    m = x.min(axis=axis)
    if tau == 0.0:
        return m
    return m - tau * np.log(np.exp(-(x - np.expand_dims(m, axis)) / tau).sum(axis=axis))


def _msg(cost, D, tau):
    """D (L, Q) -> M (L, Q): M[l, i] = (+)_j (C[i, j] + D[l, j])."""
    return oplus(cost[None, :, :] + D[:, None, :], tau)


def relatives(children):
    """(parent, sibling) dicts of a proper binary tree's child lists."""
    n_all = children.shape[0]
    nl = (n_all + 1) // 2
    parent, sibling = {}, {}
    for node in range(nl, n_all):
        c0, c1 = int(children[node, 0]), int(children[node, 1])
        parent[c0] = parent[c1] = node
        sibling[c0], sibling[c1] = c1, c0
    return parent, sibling


def nni_table_ref(children):
    """(n_int - 1, 4): (u, a0, a1, s) of v = n_leaves + e."""
    n_all = children.shape[0]
    nl = (n_all + 1) // 2
    parent, sibling = relatives(children)
    return np.array([[parent[v], children[v, 0], children[v, 1], sibling[v]]
                     for v in range(nl, n_all - 1)], dtype=np.int32).reshape(-1, 4)


def nni_ref(children, leaves, cost, tau):
    """One tree.  Returns dict: inside (n_all, L, Q), outside (n_int, L, Q),
    site_score (L,), tree_score, invariant (n_int, L) = (+)_i (O_v + D_v),
    nni (n_int - 1, 2) tree scores of the moves."""
    cost = np.asarray(cost, dtype=np.float64)
    Q = cost.shape[0]
    n_all = children.shape[0]
    nl = (n_all + 1) // 2
    ni = n_all - nl
    L = leaves.shape[1]
    D = np.zeros((n_all, L, Q))
    for x in range(nl):
        D[x] = np.where(leaves[x][:, None] == np.arange(Q)[None, :], 0.0, SENT)
    for node in range(nl, n_all):
        D[node] = _msg(cost, D[children[node, 0]], tau) + _msg(cost, D[children[node, 1]], tau)
    M = np.stack([_msg(cost, D[x], tau) for x in range(n_all)])
    parent, sibling = relatives(children)
    O = np.zeros((n_all, L, Q))
    for c in range(n_all - 2, nl - 1, -1):  # parents have higher ids
        t = O[parent[c]] + M[sibling[c]]  # (L, Qi)
        O[c] = oplus(cost[None, :, :] + t[:, :, None], tau, axis=1)
    site = oplus(D[n_all - 1], tau)
    inv = np.stack([oplus(O[v] + D[v], tau) for v in range(nl, n_all)])
    nni = np.zeros((ni - 1, 2))
    for v in range(nl, n_all - 1):
        u, s = parent[v], sibling[v]
        a = (int(children[v, 0]), int(children[v, 1]))
        for k in (0, 1):
            dv = M[s] + M[a[1 - k]]
            nni[v - nl, k] = oplus(O[u] + M[a[k]] + _msg(cost, dv, tau), tau).sum()
    return {"inside": D, "outside": O[nl:], "site_score": site, "tree_score": site.sum(),
            "invariant": inv, "nni": nni}


def hand_swap(children, v, k):
    """The neighbour's child lists with the ORIGINAL node ids (not valid under
    trex's child-below-parent rule; for leaf-set comparisons)."""
    ch = np.array(children, copy=True)
    parent, sibling = relatives(children)
    u, s = parent[v], sibling[v]
    a = (int(children[v, 0]), int(children[v, 1]))
    ch[v] = (s, a[1 - k])
    ch[u] = (a[k], v)
    return ch


def leaf_sets(children, root=None):
    """Family of leaf sets (frozensets) under every internal node reachable
    from the root, ids in any order."""
    n_all = children.shape[0]
    nl = (n_all + 1) // 2
    fam = set()

    def rec(x):
        if x < nl:
            return frozenset([x])
        s = rec(int(children[x, 0])) | rec(int(children[x, 1]))
        fam.add(s)
        return s

    rec(n_all - 1 if root is None else root)
    return fam


def apply_nni_ref(children, v, k):
    """Independent restatement of the renumbering rule: the hand-swapped tree
    with internal nodes renumbered in post-order (recursive DFS from the root,
    children in ascending id order), pairs stored ascending."""
    hs = hand_swap(children, v, k)
    n_all = hs.shape[0]
    nl = (n_all + 1) // 2
    out = np.full((n_all, 2), -1, dtype=np.int32)
    counter = [nl]

    def rec(x):
        if x < nl:
            return x
        lo, hi = sorted((int(hs[x, 0]), int(hs[x, 1])))
        n0 = rec(lo)
        n1 = rec(hi)
        me = counter[0]
        counter[0] += 1
        out[me] = (min(n0, n1), max(n0, n1))
        return me

    assert rec(n_all - 1) == n_all - 1
    return out


def brute_force(children, leaves, cost, tau):
    """(n_int - 1, 2) neighbour tree scores via rebuilt topologies + the oracle."""
    n_all = children.shape[0]
    nl = (n_all + 1) // 2
    out = np.zeros((n_all - nl - 1, 2))
    for v in range(nl, n_all - 1):
        for k in (0, 1):
            nb = apply_nni_ref(children, v, k)
            out[v - nl, k] = sankoff_fwd_bwd_ref(nb, leaves, cost, tau)["tree_score"]
    return out


def greedy_ref(children, leaves, cost, tau, min_gain=1e-5, max_rounds=100):
    """The hill climb in fp64 on one tree: steepest descent, ties to the
    lowest (v, k), move only if new < score - min_gain |score|.  Returns
    (children, history)."""
    ch = np.array(children, copy=True)
    nl = (ch.shape[0] + 1) // 2
    score = float(sankoff_fwd_bwd_ref(ch, leaves, cost, tau)["tree_score"])
    hist = [score]
    for _ in range(max_rounds):
        nb = nni_ref(ch, leaves, cost, tau)["nni"].reshape(-1)
        best = int(np.argmin(nb))
        if not nb[best] < score - min_gain * abs(score):
            break
        ch = apply_nni_ref(ch, nl + best // 2, best % 2)
        score = float(sankoff_fwd_bwd_ref(ch, leaves, cost, tau)["tree_score"])
        hist.append(score)
    return ch, hist


def _self_check():
    from _cases import int_cost, random_leaves, random_topologies

    for n, Q, tau, seed in ((5, 3, 0.0, 1), (7, 4, 0.5, 2), (6, 5, 0.0, 3)):
        ch = random_topologies(1, n, seed=seed)[0]
        lv = random_leaves(1, n, 9, Q, seed, missing=0.1 if tau == 0.0 else 0.0)[0]
        c = int_cost(Q, seed)
        if seed == 3:
            c = c + np.triu(np.ones_like(c), 1)  # asymmetric
        r = nni_ref(ch, lv, c, tau)
        bf = brute_force(ch, lv, c, tau)
        oracle = sankoff_fwd_bwd_ref(ch, lv, c, tau)
        if tau == 0.0:
            assert np.array_equal(r["nni"], bf), (r["nni"], bf)
            assert np.array_equal(r["invariant"], np.broadcast_to(r["site_score"],
                                                                   r["invariant"].shape))
            assert r["tree_score"] == oracle["tree_score"]
        else:
            np.testing.assert_allclose(r["nni"], bf, rtol=1e-12)
            np.testing.assert_allclose(r["invariant"], np.broadcast_to(
                r["site_score"], r["invariant"].shape), rtol=1e-12)
            np.testing.assert_allclose(r["tree_score"], oracle["tree_score"], rtol=1e-12)


_self_check()
