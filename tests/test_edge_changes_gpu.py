"""GPU tests of the per-branch change counts and branch lengths
(sankoff_edges.hip, SankoffEngine.edge_changes, describe_trees) against the
fp64 references of _edge_ref.py.

Shapes (n leaves, L, Q), B = 3 trees built as test_nni_gpu.case builds them:
(5, 70, 4) two tiles with a 6-lane tail, (6, 33, 3) one short tile, (7, 65, 2)
one site in the second tile, (6, 33, 5) and (5, 33, 20) the padded path at its
first and last Q.  Costs are general_cost kinds only (a symmetric cost hides a
transposed ``counts``): asym_int and asym_dyadic at tau = 0, where every
compared number is exact, asym_frac at tau = 0.5.  Leaves: int8 codes (the
asym_int tau = 0 cases carry missing codes -1, the out-of-range code) and int32
state sets with ambiguous and all-missing cells.  Weights: none, all ones
(bitwise the unweighted call), random multiples of 1/4 in [0.25, 2].

tau = 0.5, per entry: |got - ref| <= r_e ref + 1e-7 sum(w) with r_e = max(1e-5,
c 2^-24 Jmag_e / tau), c = 8 the project's constant for marginals (DESIGN.md
§4, _cases.marginal_rtol), Jmag_e from the reference.  ``lengths`` and the row
sums are linear in the counts with coefficients C_ij and 1, so their bounds
are the same combinations of the entries' bounds.  The worst err / bound of
every case is printed.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import _edge_ref as E
from _cases import general_cost, random_leaves, random_topologies
from _sets_ref import rows_from_masks
from trex_amd import EdgeChanges, SankoffEngine, TreePlan, describe_trees
from trex_amd._lib import check, lib, ptr, stream_handle

pytestmark = pytest.mark.gpu

SHAPES = [(5, 70, 4), (6, 33, 3), (7, 65, 2), (6, 33, 5), (5, 33, 20)]
HARD = [(0.0, "asym_int"), (0.0, "asym_dyadic")]
SOFT = [(0.5, "asym_frac")]
MARGINAL_C = 8.0
B = 3


def _masks(codes, Q, seed):
    """State sets from codes: 20 % of the cells get further states, 5 % are
    all-missing (every state allowed)."""
    rng = np.random.default_rng(seed)
    m = np.left_shift(1, codes.astype(np.int64))
    extra = rng.integers(0, 1 << Q, size=codes.shape)
    m = np.where(rng.random(codes.shape) < 0.2, m | extra, m)
    m = np.where(rng.random(codes.shape) < 0.05, (1 << Q) - 1, m)
    return m.astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(n, L, Q, tau, kind, sets):
    """Inputs and fp64 references, computed once per case and shared (treated
    as read-only): leaves as the device takes them, their fp64 rows, the cost,
    the quarter weights, per tree the references without and with weights, and
    at tau = 0 the first-index reconstruction and its histogram.  Asserts (CPU)
    that the reference counts tell (i, j) from (j, i) on some edge."""
    ch = random_topologies(B, n, seed=10 * n + Q)
    codes = random_leaves(B, n, L, Q, seed=n + L)
    # seed 14 for every Q: the first seed whose matrices give every tau = 0 case an
    # edge with min < max (seed Q: the Q = 3 integer matrix has the row (1, 1, 1), under
    # which the all-0 reconstruction is the only optimum; dyadic entries tie rarely)
    cost = general_cost(Q, 14, kind)
    if sets:
        leaves = _masks(codes, Q, seed=n + L + Q)
        assert ((leaves & (leaves - 1)) != 0).any() and (leaves == (1 << Q) - 1).any()
        rows = rows_from_masks(leaves, Q)
    else:
        leaves = codes.copy()
        if kind == "asym_int":  # out-of-range codes: all-1e5 rows
            leaves[0, 1, 3] = leaves[1, 0, L - 1] = leaves[2, n - 1, 0] = -1
        rows = E.rows_from_codes(leaves, Q)
    w = (np.random.default_rng(L + Q).integers(1, 9, size=(B, L)) / 4.0).astype(np.float32)
    c64 = cost.astype(np.float64)
    ref = {wk: [E.edge_ref(ch[b], rows[b], c64, tau, None if wk == "none" else w[b])
                for b in range(B)] for wk in ("none", "quarter")}
    out = dict(ch=ch, leaves=leaves, rows=rows, cost=cost, w=w, ref=ref)
    if tau == 0.0:
        out["states"] = np.stack([E.backtrack_ref(ch[b], rows[b], c64) for b in range(B)])
        cnt = np.stack([E.counts_from_states(ch[b], rows[b], c64, out["states"][b])[0]
                        for b in range(B)])
        assert any(r["length_min"][c] < r["length_max"][c] for r in ref["none"]
                   for c in range(2 * n - 2)), "no edge with min < max: another seed"
    else:
        cnt = np.stack([r["counts"] for r in ref["none"]])
    asym = np.abs(cnt - cnt.transpose(0, 1, 3, 2)).max(axis=(2, 3)) / cnt.max(axis=(2, 3)).clip(1e-300)
    assert asym.max() > 1e-2, f"counts vs transpose: {asym.max():.3e} (need > 1e-2 on some edge)"
    return out


def setup(device, k, tau):
    n_all, L = k["ch"].shape[1], k["leaves"].shape[2]
    Q = k["cost"].shape[0]
    eng = SankoffEngine(TreePlan(k["ch"]), L, Q, device)
    lv = torch.from_numpy(k["leaves"]).to(device)
    cd = torch.from_numpy(k["cost"]).to(device)
    f = eng.forward(lv, cd, tau)
    out = eng.outside(lv, cd, tau, f.dp)
    weights = {"none": None, "ones": torch.ones((B, L), device=device),
               "quarter": torch.from_numpy(k["w"]).to(device)}
    return eng, lv, cd, f, out, weights, n_all, L, Q


def host(r: EdgeChanges):
    return {name: None if t is None else t.cpu().numpy().astype(np.float64)
            for name, t in vars(r).items()}


def assert_same_bits(a: EdgeChanges, b: EdgeChanges, what):
    for name in ("counts", "lengths", "length_min", "length_max"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), name
        if x is not None:
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{what}: {name}"


def through_the_abi(eng, lv, cd, tau, dp, out, states, weights):
    """The call on outputs prefilled with NaN."""
    p = eng.plan
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=eng.device)  # noqa: E731
    hard = tau == 0.0
    r = EdgeChanges(nan(p.B, p.n_all, eng.Q, eng.Q), nan(p.B, p.n_all),
                    nan(p.B, p.n_all) if hard else None, nan(p.B, p.n_all) if hard else None)
    nb = int(lib().trex_edge_workspace_bytes(p.B, eng.L, p.n_all, eng.Q))
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=eng.device)
    fn = (lib().trex_sankoff_sets_edge_changes_w if lv.dtype == torch.int32
          else lib().trex_sankoff_edge_changes_w)
    check(fn(ptr(p.attach_device(eng.device)), ptr(lv), ptr(cd), p.B, eng.L, p.n_all, eng.Q,
             float(tau), ptr(dp), ptr(out), ptr(states), ptr(weights), ptr(r.counts),
             ptr(r.lengths), ptr(r.length_min), ptr(r.length_max), ptr(ws), nb,
             stream_handle(eng.device)))
    return r


def common_checks(eng, lv, cd, tau, f, out, weights, res, states=None):
    """What holds at every tau: shapes, the root's zeros, repeated calls, ones
    = unweighted, NaN-prefilled outputs fully written, missing tables."""
    p = eng.plan
    r = res["none"]
    assert r.counts.shape == (B, p.n_all, eng.Q, eng.Q) and r.counts.dtype == torch.float32
    assert r.lengths.shape == (B, p.n_all)
    for wk, x in res.items():
        for name in ("counts", "lengths", "length_min", "length_max"):
            t = getattr(x, name)
            assert (t is None) == (tau > 0.0 and name.startswith("length_m")), name
            if t is not None:
                assert torch.isfinite(t).all(), (wk, name)
                assert not t[:, -1].any(), f"{wk} {name}: the root's entry is 0"
        again = eng.edge_changes(lv, cd, tau, dp=f.dp, outside=out, states=states,
                                 weights=weights[wk])
        assert_same_bits(again, x, f"{wk}: two calls")
        abi = through_the_abi(eng, lv, cd, tau, f.dp, out, states if tau == 0.0 else None,
                              weights[wk])
        assert_same_bits(abi, x, f"{wk}: NaN-prefilled outputs")
    assert_same_bits(res["ones"], res["none"], "all-ones weights vs none")


@pytest.mark.parametrize("sets", [False, True], ids=["codes", "sets"])
@pytest.mark.parametrize("tau,kind", SOFT)
@pytest.mark.parametrize("n,L,Q", SHAPES)
def test_posterior_counts(device, n, L, Q, tau, kind, sets):
    k = case(n, L, Q, tau, kind, sets)
    eng, lv, cd, f, out, weights, n_all, L, Q = setup(device, k, tau)
    res = {wk: eng.edge_changes(lv, cd, tau, dp=f.dp, outside=out, weights=wt)
           for wk, wt in weights.items()}
    torch.cuda.synchronize()
    common_checks(eng, lv, cd, tau, f, out, weights, res)
    c64 = np.abs(k["cost"].astype(np.float64))
    worst = 0.0
    for wk in ("none", "quarter"):
        got = host(res[wk])
        sw = np.full(B, float(L)) if wk == "none" else k["w"].astype(np.float64).sum(axis=1)
        for b in range(B):
            ref = k["ref"][wk][b]
            r_e = np.maximum(1e-5, MARGINAL_C * 2.0 ** -24 * ref["jmag"] / tau)  # (n_all,)
            bound = r_e[:, None, None] * ref["counts"] + 1e-7 * sw[b]
            bound[-1] = 0.0
            err = np.abs(got["counts"][b] - ref["counts"])
            worst = max(worst, float((err[:-1] / bound[:-1]).max()))
            assert (err <= bound).all(), (
                f"{wk} tree {b}: counts worst err / bound {(err[:-1] / bound[:-1]).max():.3f}")
            rows_err = np.abs(got["counts"][b].sum(axis=(1, 2))[:-1] - sw[b])
            assert (rows_err <= bound.sum(axis=(1, 2))[:-1]).all(), f"{wk} tree {b}: sum_ij counts"
            len_err = np.abs(got["lengths"][b] - ref["lengths"])
            len_bound = (bound * c64[None]).sum(axis=(1, 2)) + 2.0 ** -24 * ref["lengths"]
            worst = max(worst, float((len_err[:-1] / len_bound[:-1]).max()))
            assert (len_err <= len_bound).all(), f"{wk} tree {b}: lengths"
    print(f"edge counts n={n} L={L} Q={Q} {'sets' if sets else 'codes'}: worst err / bound "
          f"{worst:.3f} (c = {MARGINAL_C:g})")
    # without tables the engine computes them; describe_trees is the same call
    assert_same_bits(eng.edge_changes(lv, cd, tau), res["none"], "missing tables")
    d = describe_trees(k["ch"], k["leaves"], k["cost"], tau=tau, weights=k["w"], device=device)
    assert_same_bits(d, res["quarter"], "describe_trees")
    with pytest.raises(ValueError):
        eng.edge_changes(lv, cd, tau, states=torch.zeros((B, n - 1, L), dtype=torch.int8,
                                                         device=device))


@pytest.mark.parametrize("sets", [False, True], ids=["codes", "sets"])
@pytest.mark.parametrize("tau,kind", HARD)
@pytest.mark.parametrize("n,L,Q", SHAPES)
def test_hard_counts_and_length_bounds_are_exact(device, n, L, Q, tau, kind, sets):
    k = case(n, L, Q, tau, kind, sets)
    eng, lv, cd, f, out, weights, n_all, L, Q = setup(device, k, tau)
    states = eng.backtrack(cd, f.dp)
    res = {wk: eng.edge_changes(lv, cd, tau, dp=f.dp, outside=out, states=states, weights=wt)
           for wk, wt in weights.items()}
    torch.cuda.synchronize()
    st = states.cpu().numpy()
    assert np.array_equal(st, k["states"]), "the engine's backtrack is the first-index one"
    common_checks(eng, lv, cd, tau, f, out, weights, res, states)
    c64 = k["cost"].astype(np.float64)
    for wk in ("none", "quarter"):
        got = host(res[wk])
        for b in range(B):
            w = None if wk == "none" else k["w"][b]
            hist, hist_len = E.counts_from_states(k["ch"][b], k["rows"][b], c64, st[b], w)
            ref = k["ref"][wk][b]
            assert np.array_equal(got["counts"][b], hist), f"{wk} tree {b}: counts"
            assert np.array_equal(got["lengths"][b], hist_len), f"{wk} tree {b}: lengths"
            assert np.array_equal(got["lengths"][b], (got["counts"][b] * c64).sum(axis=(1, 2)))
            assert np.array_equal(got["length_min"][b], ref["length_min"]), f"{wk} tree {b}: min"
            assert np.array_equal(got["length_max"][b], ref["length_max"]), f"{wk} tree {b}: max"
            assert (got["length_min"][b] <= got["lengths"][b]).all()
            assert (got["lengths"][b] <= got["length_max"][b]).all()
    # unweighted: the branch lengths add up to the forward's score, bit for bit (a
    # missing code's all-1e5 row adds exactly 1e5 to the score and nothing to a length)
    n_bad = (k["rows"].min(axis=3) > 0).sum(axis=(1, 2))
    assert (n_bad > 0).all() == (kind == "asym_int" and not sets)
    total = host(res["none"])["lengths"].sum(axis=1) + 1e5 * n_bad
    assert np.array_equal(total.astype(np.float32), f.tree_score.cpu().numpy())
    assert np.array_equal(total, f.tree_score.cpu().numpy().astype(np.float64))
    # missing states / tables: the engine's own; describe_trees is the same call
    assert_same_bits(eng.edge_changes(lv, cd, tau), res["none"], "missing tables and states")
    d = describe_trees(k["ch"], k["leaves"], k["cost"], tau=tau, weights=k["w"], device=device)
    assert_same_bits(d, res["quarter"], "describe_trees")


@pytest.mark.parametrize("sets", [False, True], ids=["codes", "sets"])
@pytest.mark.parametrize("n,L,Q", SHAPES)
def test_callers_states_are_counted_as_given(device, n, L, Q, sets):
    tau = 0.0
    k = case(n, L, Q, tau, "asym_dyadic", sets)
    eng, lv, cd, f, out, weights, n_all, L, Q = setup(device, k, tau)
    c64 = k["cost"].astype(np.float64)
    rng = np.random.default_rng(n * L)
    st = rng.integers(0, Q, size=(B, n - 1, L)).astype(np.int8)
    bad = st.copy()
    x, y = n - 2, 0  # internal rows: the root and the lowest internal node
    l0, l1 = L - 1, 1
    bad[:, x, l0] = -1
    bad[:, y, l1] = Q
    for states, holes in ((st, ()), (bad, ((x, l0), (y, l1)))):
        sd = torch.from_numpy(states).to(device)
        for wk in ("none", "quarter"):
            got = host(eng.edge_changes(lv, cd, tau, dp=f.dp, outside=out, states=sd,
                                        weights=weights[wk]))
            for b in range(B):
                w = None if wk == "none" else k["w"][b]
                hist, hist_len = E.counts_from_states(k["ch"][b], k["rows"][b], c64, states[b], w)
                assert np.array_equal(got["counts"][b], hist), f"{wk} tree {b}: counts"
                assert np.array_equal(got["lengths"][b], hist_len), f"{wk} tree {b}: lengths"
                if wk == "none":
                    # a site is missing from exactly the edges that touch the node
                    parent, _ = E.R.relatives(k["ch"][b])
                    want = np.full(n_all, float(L))
                    want[-1] = 0.0
                    for row, _site in holes:
                        node = n + row
                        for c in range(n_all - 1):
                            if c == node or parent[c] == node:
                                want[c] -= 1.0
                    assert np.array_equal(got["counts"][b].sum(axis=(1, 2)), want)
                # the bounds do not depend on the reconstruction
                assert np.array_equal(got["length_min"][b], k["ref"][wk][b]["length_min"])
                assert np.array_equal(got["length_max"][b], k["ref"][wk][b]["length_max"])
