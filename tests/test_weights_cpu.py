"""CPU tests of the site-weight host side: compress_sites, bootstrap_weights,
clade_support, the host validation of weights, and the refusals of the three
C entry points (rejected before any launch: host numpy buffers stand in for
device pointers and are never touched)."""

from __future__ import annotations

import numpy as np
import pytest

import _nni_ref as R
from _cases import random_leaves, random_topologies, simulate_leaves
from trex_amd import (apply_nni, bootstrap_weights, clade_support, compress_sites,
                      nni_hill_climb, parsimony_ratchet, stepwise_addition)
from trex_amd._lib import OPTIONAL, SIGNATURES, TREX_E_ARG, has_site_weights, lib

NEW = ("trex_site_weighted_sum", "trex_sankoff_nni_w", "trex_sankoff_attach_w")


def _check_compression(lv):
    patterns, counts, index = compress_sites(lv)
    n, L = lv.shape
    P = patterns.shape[1]
    assert patterns.dtype == np.int8 and patterns.shape == (n, P)
    assert counts.dtype == np.float32 and counts.shape == (P,)
    assert index.dtype == np.int64 and index.shape == (L,)
    assert np.array_equal(patterns[:, index], lv)  # the round trip
    assert np.array_equal(counts, np.bincount(index, minlength=P))
    assert counts.sum() == L and (counts >= 1).all()
    assert len({patterns[:, p].tobytes() for p in range(P)}) == P  # distinct columns
    # order of first occurrence: pattern p first appears after patterns 0 .. p - 1 did
    first = np.array([np.flatnonzero(index == p)[0] for p in range(P)])
    assert (np.diff(first) > 0).all() and first[0] == 0
    return patterns, counts, index


def test_compress_sites_on_the_simulated_alignment():
    lv = simulate_leaves(8, 120, 4, 6, seed=11)[0][:8]
    patterns, counts, index = _check_compression(lv)
    assert patterns.shape[1] == 44


def test_compress_sites_by_hand():
    lv = np.array([[2, 0, 2, -1, 0, -1, 2],
                   [1, 3, 1, 1, 3, 1, 0]], dtype=np.int8)
    patterns, counts, index = _check_compression(lv)
    assert np.array_equal(patterns, [[2, 0, -1, 2], [1, 3, 1, 0]])  # -1 kept as a symbol
    assert np.array_equal(counts, [2, 2, 2, 1])
    assert np.array_equal(index, [0, 1, 0, 2, 1, 2, 3])


@pytest.mark.parametrize("n,L,Q,missing", [(1, 1, 2, 0.0), (3, 200, 2, 0.0), (5, 300, 3, 0.2),
                                           (40, 50, 4, 0.0)])
def test_compress_sites_random(n, L, Q, missing):
    lv = random_leaves(1, n, L, Q, seed=n + L, missing=missing)[0]
    patterns, _, _ = _check_compression(lv)
    if missing:
        assert (patterns < 0).any()
    if (n, Q) == (3, 2):
        assert patterns.shape[1] == 8  # every one of the 2^3 columns occurs in 200 draws
    with pytest.raises(ValueError):
        compress_sites(lv[0])


def test_bootstrap_weights():
    counts = np.array([3, 0, 1, 5, 0, 2, 9], dtype=np.float32)
    w = bootstrap_weights(counts, 6, seed=4)
    assert w.shape == (6, 7) and w.dtype == np.float32
    assert np.array_equal(w.sum(axis=1), np.full(6, 20.0))
    assert not w[:, counts == 0].any()
    assert np.array_equal(w, np.floor(w)) and (w >= 0).all()
    assert np.array_equal(w, bootstrap_weights(counts, 6, seed=4))
    assert not np.array_equal(w, bootstrap_weights(counts, 6, seed=5))
    c64 = counts.astype(np.float64)
    want = np.random.default_rng(4).multinomial(20, c64 / 20, size=6)
    assert np.array_equal(w, want.astype(np.float32))
    ones = bootstrap_weights(np.ones(120), 3)
    assert ones.shape == (3, 120) and np.array_equal(ones.sum(axis=1), [120.0] * 3)
    for bad in (np.zeros(4), np.array([1.0, -1.0]), np.array([1.0, np.nan]), np.ones((2, 2))):
        with pytest.raises(ValueError):
            bootstrap_weights(bad, 2)
    with pytest.raises(ValueError):
        bootstrap_weights(counts, 0)


def test_clade_support_against_leaf_sets():
    n = 9
    ref = random_topologies(1, n, seed=5)[0]
    trees = [ref, apply_nni(ref, n, 0), apply_nni(ref, n + 3, 1), apply_nni(ref, n + 3, 1)]
    trees += list(random_topologies(3, n, seed=6))
    trees = np.stack(trees)
    fams = [R.leaf_sets(t) for t in trees]
    want = []
    for node in range(n, 2 * n - 1):
        s = max(R.leaf_sets(ref, root=node), key=len)  # the node's own leaf set
        want.append(sum(s in f for f in fams) / len(fams))
    got = clade_support(ref, trees)
    assert got.shape == (n - 1,) and got.dtype == np.float64
    assert np.array_equal(got, np.array(want))
    assert got[-1] == 1.0 and (got >= 1 / len(trees)).all() and (got <= 1.0).all()
    assert len(np.unique(got)) > 2  # the NNI moves and random trees do lose clades
    assert np.array_equal(clade_support(ref, ref), np.ones(n - 1))
    with pytest.raises(ValueError):
        clade_support(ref, random_topologies(2, n + 1, seed=1))


def test_bad_host_weights_are_rejected():
    """numpy weights are validated on the host, before any engine exists."""
    import torch

    lv = torch.zeros((5, 7), dtype=torch.int8)
    cost = np.ones((4, 4), dtype=np.float32) - np.eye(4, dtype=np.float32)
    ch = random_topologies(2, 5, seed=0)
    bad = [np.full(7, -1.0), np.full(7, np.nan), np.full(7, np.inf), np.ones(6), np.ones((3, 7)),
           np.ones((2, 7, 1)), np.array(["a"] * 7)]
    for w in bad:
        with pytest.raises(ValueError):
            stepwise_addition(lv, cost, n_trees=2, weights=w, device="cpu")
        with pytest.raises(ValueError):
            nni_hill_climb(ch, lv, cost, weights=w, device="cpu")
        with pytest.raises(ValueError):
            parsimony_ratchet(ch, lv, cost, weights=w, device="cpu")
    with pytest.raises(ValueError):
        parsimony_ratchet(ch, lv, cost, frac=1.5, device="cpu")
    with pytest.raises(ValueError):
        parsimony_ratchet(ch, lv, cost, n_iter=-1, device="cpu")


def test_entry_points_are_listed_and_optional():
    assert has_site_weights()
    for name in NEW:
        assert name in SIGNATURES and name in OPTIONAL
    assert lib().trex_version() == 10
    nni, nni_w = SIGNATURES["trex_sankoff_nni"][1], SIGNATURES["trex_sankoff_nni_w"][1]
    att, att_w = SIGNATURES["trex_sankoff_attach"][1], SIGNATURES["trex_sankoff_attach_w"][1]
    assert len(nni_w) == len(nni) + 1 and len(att_w) == len(att) + 1


def _buf(n=1 << 16):
    return np.zeros(n, np.uint8)


def test_site_weighted_sum_refusals():
    L = lib()
    p = _buf().ctypes.data
    assert L.trex_site_weighted_sum(None, p, 2, 8, p, None) == TREX_E_ARG
    assert b"null" in L.trex_last_error()
    assert L.trex_site_weighted_sum(p, None, 2, 8, p, None) == TREX_E_ARG
    assert L.trex_site_weighted_sum(p, p, 2, 8, None, None) == TREX_E_ARG
    for B in (0, -1):
        assert L.trex_site_weighted_sum(p, p, B, 8, p, None) == TREX_E_ARG
        assert b"shape" in L.trex_last_error()
    assert L.trex_site_weighted_sum(p, p, 2, 0, p, None) == TREX_E_ARG


def test_nni_w_refusals():
    L = lib()
    p = _buf().ctypes.data
    B, sites, n_all, Q = 1, 64, 7, 4
    ws = int(L.trex_nni_workspace_bytes(B, sites, n_all, Q))
    w = _buf(ws).ctypes.data
    good = [p, p, p, B, sites, n_all, Q, 0.5, p, p, p, p, w, ws, None]
    for i in (0, 1, 2, 8, 9, 11, 12):  # plan, leaves, cost, dp, outside, nni_score, workspace
        a = list(good)
        a[i] = None
        assert L.trex_sankoff_nni_w(*a) == TREX_E_ARG, i
        assert b"trex_sankoff_nni_w: null" in L.trex_last_error()
    for i, v in ((3, 0), (4, 0), (6, 1), (7, -1.0), (13, ws - 1)):  # B, L, Q, tau, workspace
        a = list(good)
        a[i] = v
        assert L.trex_sankoff_nni_w(*a) == TREX_E_ARG, i


def test_attach_w_refusals():
    L = lib()
    p = _buf().ctypes.data
    B, sites, n_all, Q = 1, 64, 7, 4
    ws = int(L.trex_attach_workspace_bytes(B, sites, n_all, Q))
    w = _buf(ws).ctypes.data
    good = [p, p, p, B, sites, n_all, Q, 0.5, p, p, p, None, p, p, w, ws, None]
    for i in (0, 1, 2, 8, 9, 13, 14):  # plan, leaves, cost, dp, outside, attach_score, workspace
        a = list(good)
        a[i] = None
        assert L.trex_sankoff_attach_w(*a) == TREX_E_ARG, i
        assert b"trex_sankoff_attach_w: null" in L.trex_last_error()
    for codes, rows in ((None, None), (p, p)):  # exactly one of sub_codes and sub_rows
        a = list(good)
        a[10], a[11] = codes, rows
        assert L.trex_sankoff_attach_w(*a) == TREX_E_ARG
        assert b"exactly one" in L.trex_last_error()
    for i, v in ((3, -2), (4, 0), (15, ws - 1)):
        a = list(good)
        a[i] = v
        assert L.trex_sankoff_attach_w(*a) == TREX_E_ARG, i
