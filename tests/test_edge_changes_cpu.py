"""Per-branch changes without a GPU: the fp64 references' self-check, the new
symbols, the host refusals of the two entry points (every call below is
rejected before any launch: host numpy buffers stand in for device pointers
and are never touched), trex_edge_workspace_bytes and to_newick."""

from __future__ import annotations

import json
import os

import numpy as np
import pytest

from _cases import weird_children
from trex_amd import EdgeChanges, children_from_adjacency, describe_trees, to_newick  # noqa: F401
from trex_amd._lib import (OPTIONAL, SIGNATURES, TREX_E_ARG, TREX_E_UNSUPPORTED, has_edge_changes,
                           lib)

ENTRY_POINTS = ("trex_sankoff_edge_changes_w", "trex_sankoff_sets_edge_changes_w")


def test_reference_self_check():
    import _edge_ref as E

    E._self_check()


def test_symbols_exist():
    L = lib()
    for name in ENTRY_POINTS + ("trex_edge_workspace_bytes",):
        assert hasattr(L, name), name
        assert name in SIGNATURES and name in OPTIONAL
    assert has_edge_changes()
    assert L.trex_version() == 10
    a, b = (SIGNATURES[n][1] for n in ENTRY_POINTS)
    assert a == b and len(a) == 19


def _buf(n=1 << 16):
    return np.zeros(n, np.uint8)


def _good(tau, Q=4):
    """A well-formed argument list (B = 1, 64 sites, 4 leaves) and the index of
    workspace_bytes in it."""
    L = lib()
    p = _buf().ctypes.data
    B, sites, n_all = 1, 64, 7
    ws = int(L.trex_edge_workspace_bytes(B, sites, n_all, min(Q, 20)))
    assert ws > 0
    w = _buf(ws).ctypes.data
    hard = p if tau == 0.0 else None
    #       0  1  2  3  4      5      6  7    8  9  10    11 12 13 14    15    16 17  18
    return [p, p, p, B, sites, n_all, Q, tau, p, p, hard, p, p, p, hard, hard, w, ws, None]


@pytest.mark.parametrize("fn_name", ENTRY_POINTS)
def test_host_refusals(fn_name):
    L = lib()
    fn = getattr(L, fn_name)
    for tau in (0.0, 0.5):
        assert fn(*_good(tau, Q=21)) == TREX_E_UNSUPPORTED
        for bad in (float("nan"), float("inf"), -1.0, -1e-30):
            a = _good(tau)
            a[7] = bad
            assert fn(*a) == TREX_E_ARG, bad
            assert b"tau" in L.trex_last_error()
        # plan, leaves, cost, dp, outside, counts, lengths, workspace
        for i in (0, 1, 2, 8, 9, 12, 13, 16):
            a = _good(tau)
            a[i] = None
            assert fn(*a) == TREX_E_ARG, (tau, i)
            assert (fn_name + ": null").encode() in L.trex_last_error()
        a = _good(tau)
        a[17] -= 1  # a workspace one byte short
        assert fn(*a) == TREX_E_ARG
        assert b"workspace too small" in L.trex_last_error()
        for i, v in ((3, 0), (4, 0), (5, 8), (6, 1)):  # B, L, n_all even, Q
            a = _good(tau)
            a[i] = v
            assert fn(*a) == TREX_E_ARG, (tau, i)
    p = _buf().ctypes.data
    for i in (10, 14, 15):  # states, length_min, length_max: all NULL at tau > 0 ...
        a = _good(0.5)
        a[i] = p
        assert fn(*a) == TREX_E_ARG, i
        assert b"states, length_min and length_max" in L.trex_last_error()
        a = _good(0.0)  # ... and all given at tau = 0
        a[i] = None
        assert fn(*a) == TREX_E_ARG, i
        assert b"states, length_min and length_max" in L.trex_last_error()


def test_workspace_bytes():
    L = lib()
    f = L.trex_edge_workspace_bytes
    for B, sites, n_all, Q in ((1, 1, 5, 2), (3, 70, 9, 4), (3, 33, 11, 3), (2, 65, 13, 5),
                               (3, 33, 9, 20), (1024, 5000, 63, 4)):
        tiles = (sites + 63) // 64
        assert f(B, sites, n_all, Q) == B * tiles * n_all * (Q * Q + 2) * 8
    assert 0.72e9 < f(1024, 5000, 63, 4) < 0.74e9
    # shapes the calls refuse
    for args in ((0, 64, 7, 4), (1, 0, 7, 4), (1, 64, 3, 4), (1, 64, 8, 4), (1, 64, 7, 1),
                 (1, 64, 7, 21), (-1, 64, 7, 4), (1, 64, 65537, 4)):
        assert f(*args) == 0, args
    # one tree's entry count tiles * n_all * (Q^2 + 2) above 2^31 - 1
    assert f(1, 64 * 84, 65535, 20) == 0  # 84 * 65535 * 402 > 2^31 - 1
    assert f(1, 64 * 81, 65535, 20) == 81 * 65535 * 402 * 8
    # the bytes of all trees computed in int64, overflow refused
    assert f(2 ** 31 - 1, 64 * 81, 65535, 20) == 0
    assert f(1 << 20, 64 * 81, 65535, 20) == (1 << 20) * 81 * 65535 * 402 * 8


def _fixture_children():
    path = os.path.join(os.path.dirname(__file__), "golden", "kat_sankoff.json")
    with open(path) as fh:
        k = json.load(fh)
    adj = np.zeros((5, 5))
    for c, p in k["adjacency_edges"]:
        adj[c, p] = 1
    return children_from_adjacency(adj)[0]


def test_to_newick_three_leaves():
    ch = _fixture_children()
    assert ch.tolist() == [[-1, -1]] * 3 + [[0, 1], [2, 3]]
    assert to_newick(ch) == "(2,(0,1));"
    assert to_newick(ch, names=["a", "b", "c"]) == "(c,(a,b));"
    ln = np.array([1.0, 0.0, 2.5, 0.125, 99.0])  # the root's entry is not written
    assert to_newick(ch, lengths=ln) == "(2:2.5,(0:1,1:0):0.125);"
    assert to_newick(ch, support=np.array([0.75, 1.0])) == "(2,(0,1)0.75)1;"
    assert to_newick(ch, ["a", "b", "c"], ln, [0.75, 1.0], fmt="%.2f") == \
        "(c:2.50,(a:1.00,b:0.00)0.75:0.12)1.00;"


def test_to_newick_five_leaves():
    # stored order is kept: node 6 lists its internal child first
    ch = np.array([[-1, -1]] * 5 + [[1, 3], [5, 0], [2, 4], [7, 6]], dtype=np.int32)
    assert to_newick(ch) == "((2,4),((1,3),0));"
    ln = np.arange(9) / 4.0
    assert to_newick(ch, lengths=ln) == \
        "((2:0.5,4:1):1.75,((1:0.25,3:0.75):1.25,0:0):1.5);"
    names = ["human", "chimp", "mouse", "gorilla", "rat"]
    sup = [0.5, 0.25, 1.0, 1.0]
    assert to_newick(ch, names, None, sup) == "((mouse,rat)1,((chimp,gorilla)0.5,human)0.25)1;"
    assert to_newick(ch, names, ln, sup) == \
        "((mouse:0.5,rat:1)1:1.75,((chimp:0.25,gorilla:0.75)0.5:1.25,human:0)0.25:1.5)1;"


@pytest.mark.parametrize("case", ["fwdref", "dag", "cycle"])
def test_to_newick_refuses_weird_children(case):
    with pytest.raises(ValueError):
        to_newick(weird_children(case))


def test_to_newick_refuses_bad_arguments():
    ch = _fixture_children()
    with pytest.raises(ValueError):
        to_newick(ch[None])
    with pytest.raises(ValueError):
        to_newick(ch, names=["a", "b"])
    with pytest.raises(ValueError):
        to_newick(ch, lengths=np.zeros(4))
    with pytest.raises(ValueError):
        to_newick(ch, support=np.zeros(3))
