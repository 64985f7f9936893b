"""fp64 numpy reference for state-set leaves (test side only; shares no code
with trex_amd).

Everything works on general leaf rows (n_leaves, L, Q): a mask's row is 0
where its bit is set and 1e5 elsewhere, a subtree's row is whatever it is.
Brute force throughout, no outside recursion: the score of a move is the
forward of the rebuilt tree (``_nni_ref.apply_nni_ref``), the score of an
attachment the forward of the grown tree (``_attach_ref.insert_leaf_ref``,
the new leaf's row appended).

``_self_check`` asserts once, at import, that singleton masks give the fp64
oracle's scores on codes, that the move and attachment scores agree with the
outside-table references of ``_nni_ref`` / ``_attach_ref`` there, and that at
tau = 0 a set-leaf site score is the minimum over the resolutions.
"""

from __future__ import annotations

import itertools

import numpy as np

import _attach_ref as A
import _nni_ref as R

SENT = 1e5


def rows_from_masks(masks, Q):
    """int masks (..., L) -> fp64 rows (..., L, Q); bits at or above Q ignored."""
    m = np.asarray(masks).astype(np.int64)
    bit = (m[..., None] >> np.arange(Q)) & 1
    return np.where(bit == 1, 0.0, SENT)


def forward_ref(children, rows, cost, tau, hard_root=False, weights=None):
    """One tree; rows (n_leaves, L, Q).  dict: inside (n_all, L, Q),
    site_score (L,), tree_score (weighted when weights (L,) are given)."""
    cost = np.asarray(cost, dtype=np.float64)
    n_all = children.shape[0]
    nl = (n_all + 1) // 2
    rows = np.asarray(rows, dtype=np.float64)
    assert rows.shape[0] == nl, (rows.shape, nl)
    D = np.zeros((n_all,) + rows.shape[1:])
    D[:nl] = rows
    for node in range(nl, n_all):
        c0, c1 = int(children[node, 0]), int(children[node, 1])
        assert 0 <= c0 < node and 0 <= c1 < node
        D[node] = R._msg(cost, D[c0], tau) + R._msg(cost, D[c1], tau)
    site = R.oplus(D[n_all - 1], 0.0 if hard_root else tau)
    w = np.ones_like(site) if weights is None else np.asarray(weights, dtype=np.float64)
    return {"inside": D, "site_score": site, "tree_score": float((w * site).sum())}


def nni_ref(children, rows, cost, tau, weights=None):
    """(n_int - 1, 2) tree scores of the moves, each by the rebuilt tree."""
    n_all = children.shape[0]
    nl = (n_all + 1) // 2
    out = np.zeros((n_all - nl - 1, 2))
    for v in range(nl, n_all - 1):
        for k in (0, 1):
            nb = R.apply_nni_ref(children, v, k)
            out[v - nl, k] = forward_ref(nb, rows, cost, tau, weights=weights)["tree_score"]
    return out


def attach_ref(children, rows, cost, tau, new_rows, weights=None):
    """(n_all,) tree scores with the subtree of inside rows ``new_rows``
    (L, Q) on the edge above every node; n_all - 1: a new root."""
    n_all = children.shape[0]
    plus = np.concatenate([np.asarray(rows, dtype=np.float64),
                           np.asarray(new_rows, dtype=np.float64)[None]])
    return np.array([forward_ref(A.insert_leaf_ref(children, x), plus, cost, tau,
                                 weights=weights)["tree_score"] for x in range(n_all)])


def _self_check():
    from _cases import general_cost, int_cost, random_leaves, random_topologies
    from oracle.softmin_ref import sankoff_fwd_bwd_ref

    for n, Q, tau, seed in ((5, 3, 0.0, 1), (7, 4, 0.5, 2), (6, 5, 0.0, 3)):
        ch = random_topologies(1, n, seed=seed)[0]
        lv = random_leaves(1, n + 1, 9, Q, seed, missing=0.1 if tau == 0.0 else 0.0)[0]
        c = int_cost(Q, seed)
        masks = np.where((lv >= 0) & (lv < Q), 1 << np.maximum(lv, 0).astype(np.int64), 0)
        rows = rows_from_masks(masks | (5 << 20), Q)  # high bits: ignored
        f = forward_ref(ch, rows[:n], c, tau)
        o = sankoff_fwd_bwd_ref(ch, lv[:n], c, tau)
        nn = nni_ref(ch, rows[:n], c, tau)
        at = attach_ref(ch, rows[:n], c, tau, rows[n])
        if tau == 0.0:
            assert f["tree_score"] == o["tree_score"]
            assert np.array_equal(nn, R.nni_ref(ch, lv[:n], c, tau)["nni"])
            assert np.array_equal(at, A.attach_ref(ch, lv[:n], c, tau, new_codes=lv[n]))
        else:
            np.testing.assert_allclose(f["tree_score"], o["tree_score"], rtol=1e-12)
            np.testing.assert_allclose(nn, R.nni_ref(ch, lv[:n], c, tau)["nni"], rtol=1e-12)
            np.testing.assert_allclose(at, A.attach_ref(ch, lv[:n], c, tau, new_codes=lv[n]),
                                       rtol=1e-12)
    # tau = 0: the minimum over all ways of choosing one allowed state per leaf
    rng = np.random.default_rng(4)
    ch = random_topologies(1, 4, seed=4)[0]
    Q, L = 3, 6
    masks = rng.integers(1, 1 << Q, size=(4, L))
    c = general_cost(Q, 4, "asym_dyadic")
    got = forward_ref(ch, rows_from_masks(masks, Q), c, 0.0)["site_score"]
    for l in range(L):
        allowed = [[s for s in range(Q) if masks[x, l] >> s & 1] for x in range(4)]
        best = min(forward_ref(ch, rows_from_masks(np.array([[1 << s] for s in pick]), Q), c,
                               0.0)["site_score"][0] for pick in itertools.product(*allowed))
        assert got[l] == best, (l, got[l], best)


_self_check()
