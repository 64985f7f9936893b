"""fp64 numpy references for the per-branch change counts and branch lengths
(test side only; shares no code with trex_amd).

Everything works on general leaf rows (n_leaves, L, Q) (``rows_from_codes``;
state sets: ``_sets_ref.rows_from_masks``).  Two independent routes:

* ``edge_ref``: the definitions -- per edge (parent p, child c, sibling s) the
  joint cost J[i][j] = O_p[i] + M_s[i] + C[i][j] + D_c[j] from inside and
  outside rows (``tables``: the recursion of ``_nni_ref.nni_ref``), the Gibbs
  pair posterior at tau > 0, the least and largest C[i][j] over the ties of
  min J at tau = 0;
* ``enumerate_ref``: every one of the Q^n_int ancestral assignments per site
  scored edge by edge, with no DP table at all: pair marginals of the Gibbs
  distribution over assignments at tau > 0, the least and largest cost of
  each edge over the optimal assignments at tau = 0.

``counts_from_states`` is the tau = 0 histogram along a given reconstruction,
``backtrack_ref`` the first-index reconstruction in fp64.
``_self_check`` asserts once, at import, that the two routes agree and that
the counts summed over the edges are the fp64 oracle's d_cost.
"""

from __future__ import annotations

import itertools

import numpy as np

import _nni_ref as R

SENT = 1e5


def rows_from_codes(codes, Q):
    """int codes (..., L) -> fp64 rows (..., L, Q): 0 at the code, 1e5
    elsewhere; a code outside [0, Q): all 1e5."""
    c = np.asarray(codes).astype(np.int64)
    return np.where(c[..., None] == np.arange(Q), 0.0, SENT)


def tables(children, rows, cost, tau):
    """One tree; rows (n_leaves, L, Q).  (D (n_all, L, Q) inside rows, M their
    messages, O (n_all, L, Q) outside rows, parent, sibling)."""
    cost = np.asarray(cost, dtype=np.float64)
    n_all = children.shape[0]
    nl = (n_all + 1) // 2
    D = np.zeros((n_all,) + rows.shape[1:])
    D[:nl] = rows
    for node in range(nl, n_all):
        D[node] = (R._msg(cost, D[children[node, 0]], tau)
                   + R._msg(cost, D[children[node, 1]], tau))
    M = np.stack([R._msg(cost, D[x], tau) for x in range(n_all)])
    parent, sibling = R.relatives(children)
    O = np.zeros_like(D)
    for c in range(n_all - 2, nl - 1, -1):
        t = O[parent[c]] + M[sibling[c]]
        O[c] = R.oplus(cost[None, :, :] + t[:, :, None], tau, axis=1)
    return D, M, O, parent, sibling


def _weights(weights, L):
    return np.ones(L) if weights is None else np.asarray(weights, dtype=np.float64)


def edge_ref(children, rows, cost, tau, weights=None):
    """One tree by the definitions.  dict: counts (n_all, Q, Q) (tau > 0),
    lengths (n_all,) (tau > 0), length_min / length_max (n_all,) (tau = 0),
    jmag (n_all,) (tau > 0: the largest |O_p[i]| + |M_s[i]| + |C_ij| + |D_c[j]|
    over the sites and the pairs whose P exceeds 2^-24), site_score (L,).
    The root's entries are 0."""
    cost = np.asarray(cost, dtype=np.float64)
    Q = cost.shape[0]
    n_all = children.shape[0]
    L = rows.shape[1]
    w = _weights(weights, L)
    D, M, O, parent, sibling = tables(children, rows, cost, tau)
    out = {"counts": np.zeros((n_all, Q, Q)), "lengths": np.zeros(n_all),
           "length_min": np.zeros(n_all), "length_max": np.zeros(n_all),
           "jmag": np.zeros(n_all), "site_score": R.oplus(D[n_all - 1], tau)}
    for c in range(n_all - 1):
        p, s = parent[c], sibling[c]
        J = (O[p] + M[s])[:, :, None] + cost[None] + D[c][:, None, :]  # (L, Qi, Qj)
        mn = J.min(axis=(1, 2), keepdims=True)
        if tau > 0.0:
            P = np.exp(-(J - mn) / tau)
            P /= P.sum(axis=(1, 2), keepdims=True)
            out["counts"][c] = (w[:, None, None] * P).sum(axis=0)
            out["lengths"][c] = (out["counts"][c] * cost).sum()
            mag = (np.abs(O[p]) + np.abs(M[s]))[:, :, None] + np.abs(cost)[None] \
                + np.abs(D[c])[:, None, :]
            out["jmag"][c] = mag[P > 2.0 ** -24].max()
        else:
            tie = J == mn
            cc = np.broadcast_to(cost[None], J.shape)
            out["length_min"][c] = (w * np.where(tie, cc, np.inf).min(axis=(1, 2))).sum()
            out["length_max"][c] = (w * np.where(tie, cc, -np.inf).max(axis=(1, 2))).sum()
    return out


def backtrack_ref(children, rows, cost):
    """tau = 0, one tree: the first-index reconstruction (n_int, L) -- the
    root takes the first argmin of its inside row, an internal child the first
    argmin over j of C[state_p][j] + D_c[j]."""
    cost = np.asarray(cost, dtype=np.float64)
    n_all = children.shape[0]
    nl = (n_all + 1) // 2
    D = tables(children, rows, cost, 0.0)[0]
    st = np.zeros((n_all - nl, rows.shape[1]), dtype=np.int64)
    st[-1] = np.argmin(D[n_all - 1], axis=1)
    for p in range(n_all - 1, nl - 1, -1):
        for c in children[p]:
            if c >= nl:
                st[c - nl] = np.argmin(cost[st[p - nl]] + D[c], axis=1)
    return st


def counts_from_states(children, rows, cost, states, weights=None):
    """tau = 0, one tree: the histogram of (parent state, child state) along
    the reconstruction ``states`` (n_int, L).  A leaf child's state is the
    first-index argmin over j of C[state_p][j] + D_c[j]; a site whose state is
    outside [0, Q) at the parent or at an internal child adds nothing to that
    edge.  (counts (n_all, Q, Q), lengths (n_all,))."""
    cost = np.asarray(cost, dtype=np.float64)
    Q = cost.shape[0]
    n_all = children.shape[0]
    nl = (n_all + 1) // 2
    L = rows.shape[1]
    w = _weights(weights, L)
    st = np.asarray(states).astype(np.int64)
    counts = np.zeros((n_all, Q, Q))
    for p in range(nl, n_all):
        for c in (int(children[p, 0]), int(children[p, 1])):
            for l in range(L):
                sp = st[p - nl, l]
                if not 0 <= sp < Q:
                    continue
                if c < nl:
                    sc = int(np.argmin(cost[sp] + rows[c, l]))
                else:
                    sc = st[c - nl, l]
                    if not 0 <= sc < Q:
                        continue
                counts[c, sp, sc] += w[l]
    return counts, (counts * cost[None]).sum(axis=(1, 2))


def enumerate_ref(children, rows, cost, tau, weights=None):
    """One tree by exhaustive enumeration of all Q^n_int ancestral
    assignments per site; no inside or outside rows.  An assignment's cost is
    the sum over the internal edges of C[a_p][a_c] plus, per leaf edge, (+)_j
    (C[a_p][j] + D_c[j]).  tau > 0: counts = the pair marginals of the Gibbs
    distribution (a leaf's state j given a_p: softmax_j of -(C[a_p][j] +
    D_c[j]) / tau).  tau = 0: length_min / length_max = the least / largest
    cost of the edge over the optimal assignments (a leaf edge: over the j
    that attain its minimum).  Same dict as ``edge_ref`` without jmag."""
    cost = np.asarray(cost, dtype=np.float64)
    Q = cost.shape[0]
    n_all = children.shape[0]
    nl = (n_all + 1) // 2
    ni = n_all - nl
    L = rows.shape[1]
    w = _weights(weights, L)
    leaf_x = {c: cost[None, :, :] + rows[c][:, None, :] for c in range(nl)}  # (L, Qi, Qj)
    leaf_m = {c: R.oplus(leaf_x[c], tau) for c in range(nl)}                # (L, Qi)
    edges = [(p, int(c)) for p in range(nl, n_all) for c in children[p]]
    assigns = list(itertools.product(range(Q), repeat=ni))
    E = np.zeros((len(assigns), L))
    for t, a in enumerate(assigns):
        for p, c in edges:
            sp = a[p - nl]
            E[t] += leaf_m[c][:, sp] if c < nl else cost[sp, a[c - nl]]
    emin = E.min(axis=0)
    out = {"counts": np.zeros((n_all, Q, Q)), "lengths": np.zeros(n_all),
           "length_min": np.zeros(n_all), "length_max": np.zeros(n_all)}
    if tau > 0.0:
        g = np.exp(-(E - emin) / tau)
        z = g.sum(axis=0)
        g /= z
        out["site_score"] = emin - tau * np.log(z)
        for t, a in enumerate(assigns):
            for p, c in edges:
                sp = a[p - nl]
                if c < nl:
                    x = leaf_x[c][:, sp, :]
                    cond = np.exp(-(x - x.min(axis=1, keepdims=True)) / tau)
                    cond /= cond.sum(axis=1, keepdims=True)
                    out["counts"][c, sp] += ((w * g[t])[:, None] * cond).sum(axis=0)
                else:
                    out["counts"][c, sp, a[c - nl]] += (w * g[t]).sum()
        out["lengths"] = (out["counts"] * cost[None]).sum(axis=(1, 2))
        return out
    out["site_score"] = emin
    lo = np.full((n_all, L), np.inf)
    hi = np.full((n_all, L), -np.inf)
    for t, a in enumerate(assigns):
        opt = E[t] == emin
        for p, c in edges:
            sp = a[p - nl]
            if c < nl:
                x = leaf_x[c][:, sp, :]
                tie = x == x.min(axis=1, keepdims=True)
                cl = np.where(tie, cost[sp][None, :], np.inf).min(axis=1)
                ch = np.where(tie, cost[sp][None, :], -np.inf).max(axis=1)
            else:
                cl = ch = np.full(L, cost[sp, a[c - nl]])
            lo[c] = np.where(opt, np.minimum(lo[c], cl), lo[c])
            hi[c] = np.where(opt, np.maximum(hi[c], ch), hi[c])
    out["length_min"][:n_all - 1] = (w * lo[:n_all - 1]).sum(axis=1)
    out["length_max"][:n_all - 1] = (w * hi[:n_all - 1]).sum(axis=1)
    return out


def _self_check():
    from _cases import general_cost, random_leaves, random_topologies
    from _sets_ref import rows_from_masks
    from oracle.softmin_ref import sankoff_fwd_bwd_ref

    for n, Q, L, tau, kind, seed in ((4, 2, 6, 0.0, "asym_int", 1), (5, 3, 5, 0.0, "asym_dyadic", 2),
                                     (4, 3, 6, 0.5, "asym_frac", 3), (5, 2, 4, 0.5, "asym_frac", 4),
                                     (5, 3, 4, 0.0, "asym_int", 5)):
        ch = random_topologies(1, n, seed=seed)[0]
        lv = random_leaves(1, n, L, Q, seed)[0]
        cost = general_cost(Q, seed, kind, hi=2 if seed == 5 else None).astype(np.float64)
        w = np.random.default_rng(seed).integers(1, 9, size=L) / 4.0
        rows = rows_from_codes(lv, Q)
        D, _, O, _, _ = tables(ch, rows, cost, tau)
        nn = R.nni_ref(ch, lv, cost, tau)
        assert np.array_equal(D, nn["inside"]) and np.array_equal(O[n:], nn["outside"])
        if seed in (2, 4):  # state sets with ambiguous and all-missing cells, a missing code
            rng = np.random.default_rng(seed)
            masks = (1 << lv.astype(np.int64)) | rng.integers(0, 1 << Q, size=lv.shape) \
                * (rng.random(lv.shape) < 0.3)
            masks[0, 0] = (1 << Q) - 1
            rows = rows_from_masks(masks, Q)
            rows[1, 1] = SENT  # an out-of-range code's row
        for wt in (None, w):
            a = edge_ref(ch, rows, cost, tau, wt)
            b = enumerate_ref(ch, rows, cost, tau, wt)
            np.testing.assert_allclose(a["site_score"], b["site_score"], rtol=1e-12)
            for key in ("counts", "lengths", "length_min", "length_max"):
                np.testing.assert_allclose(a[key], b[key], rtol=1e-12, atol=1e-12, err_msg=key)
            if tau == 0.0:
                assert np.array_equal(a["length_min"], b["length_min"])
                assert np.array_equal(a["length_max"], b["length_max"])
                assert (a["length_min"] <= a["length_max"]).all()
        if tau > 0.0 and seed == 3:
            o = sankoff_fwd_bwd_ref(ch, lv, cost, tau)
            np.testing.assert_allclose(edge_ref(ch, rows, cost, tau)["counts"].sum(axis=0),
                                       o["d_cost"], rtol=1e-12)
            np.testing.assert_allclose(enumerate_ref(ch, rows, cost, tau)["counts"].sum(axis=0),
                                       o["d_cost"], rtol=1e-12)
        if tau == 0.0:
            # along any optimal reconstruction an edge's cost lies in [min, max] and
            # the edge costs sum to the score
            cnt, ln = counts_from_states(ch, rows, cost, backtrack_ref(ch, rows, cost))
            a = edge_ref(ch, rows, cost, tau)
            assert (a["length_min"] <= ln).all() and (ln <= a["length_max"]).all()
            clean = rows.min(axis=2).max() == 0.0  # no all-1e5 leaf row
            if clean:
                assert ln.sum() == a["site_score"].sum()


_self_check()
