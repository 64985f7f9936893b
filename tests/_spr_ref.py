"""fp64 numpy references for the SPR neighbour scores (test side only; shares
no code with trex_amd).

Move (v, x) of a tree T: v any node but the root, u its parent, s its sibling.
Prune: u disappears and s takes its place (u the root: s is the root of T\\v).
Regraft: a new node w with children {x, v} goes on the edge above x, any node
of T\\v (x not in subtree(v), x != u).  Two independent routes to its score:

* ``spr_ref``: the definitions -- T's inside and outside rows, per pruned node
  the changed inside rows D' on u's proper ancestors, the outside rows O' of
  T\\v top-down, then the attachment score of M_v on the edge above x;
* ``brute_force``: the neighbour's child lists rebuilt explicitly
  (``apply_spr_ref``), then the fp64 oracle's tree score
  (oracle.softmin_ref.sankoff_fwd_bwd_ref).

``_self_check`` asserts once, at import, that the two agree, the +inf mask of
the moves that do not exist, and the two identities: entry (v, sibling(v)) is
the tree's own score, and NNI move (v, k) is SPR entry (s, a_(1-k)) and entry
(a_(1-k), s).
"""

from __future__ import annotations

import numpy as np

from _nni_ref import SENT, _msg, nni_ref, oplus, relatives
from oracle.softmin_ref import sankoff_fwd_bwd_ref


def leaf_rows(codes, Q):
    """(n, L) codes -> (n, L, Q) inside rows: 0 at the code, 1e5 elsewhere."""
    codes = np.asarray(codes)
    return np.where(codes[:, :, None] == np.arange(Q)[None, None, :], 0.0, SENT)


def mask_rows(masks, Q):
    """(n, L) int32 state sets -> (n, L, Q) inside rows: 0 where bit j is set."""
    masks = np.asarray(masks).astype(np.int64)
    return np.where((masks[:, :, None] >> np.arange(Q)[None, None, :]) & 1, 0.0, SENT)


def subtree(children, v):
    """Node ids of subtree(v), v included."""
    nl = (children.shape[0] + 1) // 2
    out, todo = set(), [int(v)]
    while todo:
        x = todo.pop()
        out.add(x)
        if x >= nl:
            todo.extend(int(c) for c in children[x])
    return out


def valid_mask(children):
    """(n_all - 1, n_all) bool: move (v, x) exists."""
    n_all = children.shape[0]
    parent, _ = relatives(children)
    ok = np.ones((n_all - 1, n_all), dtype=bool)
    for v in range(n_all - 1):
        ok[v, sorted(subtree(children, v))] = False
        ok[v, parent[v]] = False
    return ok


def spr_ref(children, leaves, cost, tau):
    """One tree.  leaves: (n_leaves, L) codes or (n_leaves, L, Q) inside rows
    (so masks are served too).  Returns (n_all - 1, n_all) fp64 tree scores of
    the moves (v, x), +inf where the move does not exist."""
    cost = np.asarray(cost, dtype=np.float64)
    Q = cost.shape[0]
    n_all = children.shape[0]
    nl = (n_all + 1) // 2
    leaves = np.asarray(leaves)
    rows = leaf_rows(leaves, Q) if leaves.ndim == 2 else leaves.astype(np.float64)
    L = rows.shape[1]
    root = n_all - 1
    D = np.zeros((n_all, L, Q))
    D[:nl] = rows
    for node in range(nl, n_all):
        D[node] = _msg(cost, D[children[node, 0]], tau) + _msg(cost, D[children[node, 1]], tau)
    M = np.stack([_msg(cost, D[x], tau) for x in range(n_all)])
    parent, sibling = relatives(children)
    O = np.zeros((n_all, L, Q))
    for c in range(n_all - 2, nl - 1, -1):
        t = O[parent[c]] + M[sibling[c]]
        O[c] = oplus(cost[None, :, :] + t[:, :, None], tau, axis=1)
    out = np.full((n_all - 1, n_all), np.inf)
    for v in range(n_all - 1):
        u, s = parent[v], sibling[v]
        gone = subtree(children, v) | {u}
        par2 = {y: parent[y] for y in range(n_all) if y not in gone and y != root}
        sib2 = {y: sibling[y] for y in par2}
        if u == root:
            root2 = s
            del par2[s], sib2[s]
        else:
            root2 = root
            g, t = parent[u], sibling[u]
            par2[s], sib2[s], sib2[t] = g, t, s
        # inside rows of T\v: changed on the proper ancestors of u, bottom-up
        D2, M2 = {}, {}
        P = []
        if u != root:
            D2[g] = M[s] + M[t]
            P.append(g)
            y = g
            while y != root:
                py = parent[y]
                D2[py] = _msg(cost, D2[y], tau) + M[sibling[y]]
                P.append(py)
                y = py
        for y in P:
            M2[y] = _msg(cost, D2[y], tau)
        m2 = lambda y: M2[y] if y in M2 else M[y]  # noqa: E731
        # outside rows of T\v: O on P, 0 at its root, else top-down
        O2 = {y: O[y] for y in P}
        O2[root2] = np.zeros((L, Q))
        for y in sorted(par2, reverse=True):  # parents have higher ids
            if y in O2 or y < nl:
                continue
            t2 = O2[par2[y]] + m2(sib2[y])
            O2[y] = oplus(cost[None, :, :] + t2[:, :, None], tau, axis=1)
        for x in range(n_all):
            if x in gone:
                continue
            if x == root2:
                site = oplus(m2(x) + M[v], tau)
            else:
                site = oplus(O2[par2[x]] + m2(sib2[x]) + _msg(cost, m2(x) + M[v], tau), tau)
            out[v, x] = site.sum()
    return out


def apply_spr_ref(children, v, x):
    """Independent restatement of the neighbour's child lists: s stands where
    u stood, the new node w (id n_all here) where x stood, with children
    {x, v}; internal nodes renumbered in post-order by a recursive DFS from
    the root that visits children in ascending order of their old ids, w
    taking x's place in that order; pairs stored ascending."""
    children = np.asarray(children)
    n_all = children.shape[0]
    nl = (n_all + 1) // 2
    parent, sibling = relatives(children)
    assert 0 <= v < n_all - 1 and 0 <= x < n_all
    u, s = parent[v], sibling[v]
    assert x != u and x not in subtree(children, v), (v, x)
    W = n_all

    def kids(node):
        if node == W:
            return [x, v]
        pair = []
        for c in (int(children[node, 0]), int(children[node, 1])):
            c = s if c == u else c
            pair.append(W if c == x else c)
        return pair

    root = n_all - 1
    if u == root:
        root = s
    if x == root:
        root = W
    order = lambda c: (x, 1) if c == W else (c, 0)  # noqa: E731
    out = np.full((n_all, 2), -1, dtype=np.int32)
    counter = [nl]

    def rec(node):
        if node < nl:
            return node
        lo, hi = sorted(kids(node), key=order)
        n0 = rec(lo)
        n1 = rec(hi)
        me = counter[0]
        counter[0] += 1
        out[me] = (min(n0, n1), max(n0, n1))
        return me

    assert rec(root) == n_all - 1
    return out


def brute_force(children, leaves, cost, tau):
    """(n_all - 1, n_all) neighbour tree scores via rebuilt topologies + the
    oracle (leaves: (n_leaves, L) codes); +inf where the move does not exist."""
    n_all = children.shape[0]
    ok = valid_mask(children)
    out = np.full((n_all - 1, n_all), np.inf)
    for v in range(n_all - 1):
        for x in range(n_all):
            if ok[v, x]:
                nb = apply_spr_ref(children, v, x)
                out[v, x] = sankoff_fwd_bwd_ref(nb, leaves, cost, tau)["tree_score"]
    return out


def greedy_ref(children, leaves, cost, tau, min_gain=1e-5, max_rounds=100):
    """The SPR hill climb in fp64 on one tree: steepest descent, ties to the
    lowest flattened (v, x), move only if new < score - min_gain |score|.
    Returns (children, history)."""
    ch = np.array(children, copy=True)
    n_all = ch.shape[0]
    score = float(sankoff_fwd_bwd_ref(ch, leaves, cost, tau)["tree_score"])
    hist = [score]
    for _ in range(max_rounds):
        nb = spr_ref(ch, leaves, cost, tau).reshape(-1)
        best = int(np.argmin(nb))
        if not nb[best] < score - min_gain * abs(score):
            break
        ch = apply_spr_ref(ch, best // n_all, best % n_all)
        score = float(sankoff_fwd_bwd_ref(ch, leaves, cost, tau)["tree_score"])
        hist.append(score)
    return ch, hist


def identity_pairs(children):
    """[(v, k, (s, a), (a, s))] with a = a_(1-k): NNI move (v, k) of
    _nni_ref and its two SPR entries."""
    n_all = children.shape[0]
    nl = (n_all + 1) // 2
    _, sibling = relatives(children)
    out = []
    for v in range(nl, n_all - 1):
        for k in (0, 1):
            a = int(children[v, 1 - k])
            out.append((v, k, (sibling[v], a), (a, sibling[v])))
    return out


def _self_check():
    from _cases import int_cost, random_leaves, random_topologies

    cat6 = np.array([[-1, -1]] * 6 + [[0, 1], [2, 6], [3, 7], [4, 8], [5, 9]], dtype=np.int32)
    for n, Q, tau, seed in ((5, 3, 0.0, 1), (7, 4, 0.5, 2), (6, 5, 0.0, 3), (6, 4, 0.5, 4)):
        ch = cat6 if seed == 4 else random_topologies(1, n, seed=seed)[0]
        lv = random_leaves(1, n, 9, Q, seed, missing=0.1 if tau == 0.0 else 0.0)[0]
        c = int_cost(Q, seed)
        if seed >= 3:
            c = c + np.triu(np.ones_like(c), 1)  # asymmetric
        parent, sibling = relatives(ch)
        if seed == 4:  # leaf 5 and node 9 hang off the root: pruned with u the root
            assert parent[5] == parent[9] == 2 * n - 2
        r = spr_ref(ch, lv, c, tau)
        bf = brute_force(ch, lv, c, tau)
        ok = valid_mask(ch)
        assert np.array_equal(np.isinf(r), ~ok) and np.array_equal(np.isinf(bf), ~ok)
        nni = nni_ref(ch, lv, c, tau)
        own = np.array([r[v, sibling[v]] for v in range(2 * n - 2)])
        pairs = identity_pairs(ch)
        if tau == 0.0:
            assert np.array_equal(r, bf), (r, bf)
            assert (own == nni["tree_score"]).all()
            for v, k, e0, e1 in pairs:
                assert r[e0] == r[e1] == nni["nni"][v - n, k], (v, k)
        else:
            np.testing.assert_allclose(r[ok], bf[ok], rtol=1e-12)
            np.testing.assert_allclose(own, nni["tree_score"], rtol=1e-12)
            for v, k, e0, e1 in pairs:
                np.testing.assert_allclose([r[e0], r[e1]], nni["nni"][v - n, k], rtol=1e-12)


_self_check()
