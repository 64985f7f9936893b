"""GPU tests of the site weights: the weighted total of a forward pass
(site_weights.hip), weighted NNI and attachment scores (sankoff_nni.hip),
pattern compression, the weighted searches, the ratchet, the bootstrap, guard
bands and refusals.

The reference for integer weights is the unweighted problem on the alignment
with column l repeated w_l times (``np.repeat(leaves, w, axis=1)``; weight 0
drops the column), scored by the fp64 references of _nni_ref.py and
_attach_ref.py as they are.  For fractional weights it is ``sum_l w_l *
ref(column l alone)`` in fp64.  Hard mode with integer costs and integer
weights is exact; softmin keeps the kernels' 1e-5 relative bar (weights > 0:
nothing cancels)."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import _attach_ref as A
import _guard as G
import _nni_ref as R
from _cases import general_cost, random_leaves, random_topologies, simulate_leaves
from test_nni_gpu import SHAPES, case as nni_case
from trex_amd import (SankoffEngine, TreePlan, apply_nni, bootstrap_search, bootstrap_weights,
                      clade_support, compress_sites, nni_hill_climb, parsimony_ratchet,
                      parsimony_search, stepwise_addition)

pytestmark = pytest.mark.gpu

B = 3
BIG = 1000.0  # one tree's weight on site L - 1: a clamped tail lane that leaks shows up


def int_weights(nb, L, seed):
    """(nb, L) float32 integers in 0..3 (>= 1 where L = 1), tree 1: BIG on the
    last site -- the site every lane past L reads."""
    w = np.random.default_rng(seed).integers(0, 4, size=(nb, L))
    if L == 1:
        w = np.maximum(w, 1)
    w[1, L - 1] = BIG
    return w.astype(np.float32)


def frac_weights(nb, L, seed):
    return np.random.default_rng(seed).uniform(0.25, 2.0, size=(nb, L)).astype(np.float32)


def expand(x, w, axis):
    """column l of x repeated w_l times"""
    return np.repeat(x, np.asarray(w).astype(np.int64), axis=axis)


def dev(x, device):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device)


def rel_err(got, want):
    return float((np.abs(got.astype(np.float64) - want) / np.abs(want)).max())


# ---------------------------------------------------------------------------
# 1. the weighted total
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 63, 64, 65, 257, 1000])
def test_weighted_total(device, L):
    n, Q = 5, 4
    ch = random_topologies(B, n, seed=L)
    lv = random_leaves(B, n, L, Q, seed=L + 1)
    cost = general_cost(Q, 3, "asym_int")
    eng = SankoffEngine(TreePlan(ch), L, Q, device)
    lvd, cd = dev(lv, device), dev(cost, device)
    plain = eng.forward(lvd, cd, 0.0, site_score=True)
    ss = plain.site_score.cpu().numpy().astype(np.float64)

    ones = torch.ones((B, L), dtype=torch.float32, device=device)
    f = eng.forward(lvd, cd, 0.0, weights=ones)
    assert torch.equal(f.tree_score, plain.tree_score), "all-ones weights"
    assert torch.equal(f.site_score, plain.site_score) and torch.equal(f.dp, plain.dp)
    assert torch.equal(eng.weighted_score(plain.site_score, ones), plain.tree_score)

    wi = int_weights(B, L, seed=L + 2)
    want = (wi.astype(np.float64) * ss).sum(axis=1)
    assert want.max() < 2 ** 24  # integers exact in fp32
    got = eng.weighted_score(plain.site_score, dev(wi, device))
    assert got.shape == (B,) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().astype(np.float64), want), "integer weights"
    assert torch.equal(eng.forward(lvd, cd, 0.0, weights=dev(wi, device)).tree_score, got)

    wf = frac_weights(B, L, seed=L + 3)
    wfd = dev(wf, device)
    want = (wf.astype(np.float64) * ss).sum(axis=1)  # products exact, the sum errs by L 2^-53
    got = eng.weighted_score(plain.site_score, wfd)
    err = rel_err(got.cpu().numpy(), want)
    print(f"weighted total L={L}: worst rel err {err:.3e} (bar 2^-23 = {2.0 ** -23:.3e})")
    assert err <= 2.0 ** -23
    out = torch.full((B,), -1.0, dtype=torch.float32, device=device)
    assert eng.weighted_score(plain.site_score, wfd, out=out) is out
    assert torch.equal(out, got), "repeated calls"


@pytest.mark.parametrize("Q,tau,hard_root", [(2, 0.5, False), (4, 0.5, True), (20, 0.5, False),
                                             (20, 0.0, False), (61, 0.5, False),
                                             (100, 0.0, False)])
def test_forward_with_weights_for_every_q(device, Q, tau, hard_root):
    n, L = 6, 70
    ch = random_topologies(B, n, seed=Q)
    lvd = dev(random_leaves(B, n, L, Q, seed=Q + 1), device)
    cd = dev(general_cost(Q, 2, "asym_frac" if tau else "asym_int"), device)
    w = dev(frac_weights(B, L, seed=Q), device)
    eng = SankoffEngine(TreePlan(ch), L, Q, device)
    plain = eng.forward(lvd, cd, tau, site_score=True, hard_root=hard_root)
    f = eng.forward(lvd, cd, tau, hard_root=hard_root, weights=w)
    assert torch.equal(f.site_score, plain.site_score) and torch.equal(f.dp, plain.dp)
    assert torch.equal(f.tree_score, eng.weighted_score(plain.site_score, w))
    want = (w.double() * plain.site_score.double()).sum(dim=1)
    assert rel_err(f.tree_score.cpu().numpy(), want.cpu().numpy()) <= 2.0 ** -23
    assert not torch.equal(f.tree_score, plain.tree_score)


# ---------------------------------------------------------------------------
# 2 - 4. NNI and attachment scores
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def attach_inputs(n, L, Q, tau):
    """The new leaf (B, L) int8 and a subtree's root rows (B, L, Q) float32 (a
    3-leaf tree's fp64 inside row, rounded: an input like any other); missing
    codes where test_nni_gpu's case has them."""
    missing = 0.05 if (tau == 0.0 and n == 6) else 0.0
    cost = nni_case(n, L, Q, tau)[2]
    new = np.ascontiguousarray(random_leaves(B, 1, L, Q, seed=7 * n + L, missing=missing)[:, 0])
    chs = random_topologies(B, 3, seed=n + Q)
    lvs = random_leaves(B, 3, L, Q, seed=9 * n + L)
    rows = np.stack([R.nni_ref(chs[b], lvs[b], cost, tau)["inside"][-1] for b in range(B)])
    return new, np.ascontiguousarray(rows.astype(np.float32))


def ref_scores(kind, ch, lv, cost, tau, new=None, rows=None):
    """fp64 scores of one tree: nni (n_int - 1, 2), leaf / rows (n_all,)"""
    if kind == "nni":
        return R.nni_ref(ch, lv, cost, tau)["nni"]
    if kind == "leaf":
        return A.attach_ref(ch, lv, cost, tau, new_codes=new)
    return A.attach_ref(ch, lv, cost, tau, sub_rows=rows.astype(np.float64))


@functools.lru_cache(maxsize=None)
def expanded_ref(kind, n, L, Q, tau, seed):
    """Integer weights and the reference on the expanded alignment (the
    subtree's columns repeated too), per tree."""
    ch, lv, cost, _ = nni_case(n, L, Q, tau)
    new, rows = attach_inputs(n, L, Q, tau)
    w = int_weights(B, L, seed)
    ref = np.stack([ref_scores(kind, ch[b], expand(lv[b], w[b], 1), cost, tau,
                               expand(new[b], w[b], 0), expand(rows[b], w[b], 0))
                    for b in range(B)])
    return w, ref


@functools.lru_cache(maxsize=None)
def column_ref(kind, n, L, Q, tau, seed, integer=False):
    """Weights and sum_l w_l * ref(column l alone) in fp64, per tree."""
    ch, lv, cost, _ = nni_case(n, L, Q, tau)
    new, rows = attach_inputs(n, L, Q, tau)
    w = int_weights(B, L, seed) if integer else frac_weights(B, L, seed)
    ref = np.stack([sum(float(w[b, l]) * ref_scores(kind, ch[b], lv[b][:, l:l + 1], cost, tau,
                                                    new[b][l:l + 1], rows[b][l:l + 1])
                        for l in range(L)) for b in range(B)])
    return w, ref


def device_scores(device, kind, n, L, Q, tau, w):
    ch, lv, cost, _ = nni_case(n, L, Q, tau)
    new, rows = attach_inputs(n, L, Q, tau)
    eng = SankoffEngine(TreePlan(ch), L, Q, device)
    lvd, cd = dev(lv, device), dev(cost, device)
    wd = None if w is None else dev(w, device)
    f = eng.forward(lvd, cd, tau)
    out = eng.outside(lvd, cd, tau, f.dp)
    if kind == "nni":
        return eng.nni_scores(lvd, cd, tau, dp=f.dp, outside=out, weights=wd)
    sub = dict(new_leaf=dev(new, device)) if kind == "leaf" else dict(sub_rows=dev(rows, device))
    return eng.attach_scores(lvd, cd, tau, dp=f.dp, outside=out, weights=wd, **sub)


KINDS = ["nni", "leaf", "rows"]


@pytest.mark.parametrize("n,L,Q", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_hard_mode_is_exact_on_the_expanded_alignment(device, kind, n, L, Q):
    w, ref = expanded_ref(kind, n, L, Q, 0.0, seed=n + L)
    assert (w == 0).any() or L == 1
    assert w[1, L - 1] == BIG and float(ref.max()) < 2 ** 24  # integers exact in fp32
    got = device_scores(device, kind, n, L, Q, 0.0, w)
    assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape
    assert torch.equal(got.cpu(), torch.from_numpy(ref.astype(np.float32))), kind
    assert torch.equal(device_scores(device, kind, n, L, Q, 0.0, w), got), "repeated calls"


@pytest.mark.parametrize("n,L,Q", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tau", [0.0, 0.5])
def test_all_ones_weights_are_bitwise_neutral(device, kind, tau, n, L, Q):
    plain = device_scores(device, kind, n, L, Q, tau, None)
    ones = device_scores(device, kind, n, L, Q, tau, np.ones((B, L), np.float32))
    G.assert_bitwise(ones, plain, f"{kind}: all-ones weights vs no weights")


@pytest.mark.parametrize("n,L,Q", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_softmin_within_1e5_of_the_fp64_column_reference(device, kind, n, L, Q):
    tau = 0.5
    w, ref = column_ref(kind, n, L, Q, tau, seed=n + L + 1)
    assert w.min() >= 0.25  # positive: nothing cancels
    got = device_scores(device, kind, n, L, Q, tau, w).cpu().numpy()
    err = rel_err(got, ref)
    print(f"weighted softmin {kind} n={n} L={L} Q={Q}: worst rel err {err:.3e}")
    assert err <= 1e-5, f"{kind}: worst rel err {err:.3e}"


def test_the_column_reference_agrees_with_brute_force_on_integer_weights():
    """The fp64 per-column reference against the fp64 oracle on rebuilt trees
    over the expanded alignment (reference side only)."""
    n, L, Q, tau = 6, 70, 4, 0.5
    ch, lv, cost, _ = nni_case(n, L, Q, tau)
    new, _ = attach_inputs(n, L, Q, tau)
    w, nni = column_ref("nni", n, L, Q, tau, 5, integer=True)
    _, leaf = column_ref("leaf", n, L, Q, tau, 5, integer=True)
    for b in range(B):
        lx, nx = expand(lv[b], w[b], 1), expand(new[b], w[b], 0)
        assert rel_err(nni[b], R.brute_force(ch[b], lx, cost, tau)) <= 1e-5
        bf = A.brute_force(ch[b], np.concatenate([lx, nx[None]]), cost, tau)
        assert rel_err(leaf[b], bf) <= 1e-5


# ---------------------------------------------------------------------------
# 5. compression
# ---------------------------------------------------------------------------
def alignment():
    return np.ascontiguousarray(simulate_leaves(8, 120, 4, 6, seed=11)[0][:8])


@pytest.mark.parametrize("tau", [0.0, 0.5])
def test_compressed_alignment_scores_like_the_full_one(device, tau):
    lv = alignment()
    patterns, counts, _ = compress_sites(lv)
    P = patterns.shape[1]
    assert P == 44
    cost = general_cost(4, 1, "asym_int" if tau == 0.0 else "asym_frac")
    cd = dev(cost, device)
    wd = dev(np.tile(counts, (B, 1)), device)
    worst = 0.0

    def compare(a, b, what):
        nonlocal worst
        if tau == 0.0:
            G.assert_bitwise(a, b, what)
        else:
            err = rel_err(a.cpu().numpy(), b.cpu().numpy().astype(np.float64))
            worst = max(worst, err)
            assert err <= 1e-5, f"{what}: worst rel err {err:.3e}"

    for n in (8, 7):  # 8: forward and NNI; 7: taxon 7 attached on every edge of 7-taxon trees
        ch = random_topologies(B, n, seed=13 + n)
        full = dev(np.tile(lv[None, :n], (B, 1, 1)), device)
        comp = dev(np.tile(patterns[None, :n], (B, 1, 1)), device)
        ef = SankoffEngine(TreePlan(ch), 120, 4, device)
        ec = SankoffEngine(TreePlan(ch), P, 4, device)
        if n == 8:
            compare(ec.forward(comp, cd, tau, weights=wd).tree_score,
                    ef.forward(full, cd, tau).tree_score, "forward")
            compare(ec.nni_scores(comp, cd, tau, weights=wd), ef.nni_scores(full, cd, tau), "nni")
        else:
            new_f = dev(np.tile(lv[None, 7], (B, 1)), device)
            new_c = dev(np.tile(patterns[None, 7], (B, 1)), device)
            compare(ec.attach_scores(comp, cd, tau, new_leaf=new_c, weights=wd),
                    ef.attach_scores(full, cd, tau, new_leaf=new_f), "attach")
    if tau:
        print(f"compressed vs full alignment, softmin: worst rel err {worst:.3e}")


# ---------------------------------------------------------------------------
# 6 - 8. search, ratchet, bootstrap (hard mode, integer costs)
# ---------------------------------------------------------------------------
def weighted_forward(device, ch, lv, cost, w, tau=0.0):
    nb = len(ch)
    lvd = dev(lv, device)[None].expand(nb, -1, -1).contiguous()
    wd = dev(np.broadcast_to(w, (nb, lv.shape[1])).astype(np.float32), device)
    eng = SankoffEngine(TreePlan(ch), lv.shape[1], cost.shape[0], device)
    return eng.forward(lvd, dev(cost, device), tau, weights=wd).tree_score.cpu().numpy()


def test_hill_climb_equals_the_fp64_greedy_on_the_expanded_alignment(device):
    lv = alignment()
    cost = general_cost(4, 1, "asym_int")
    ch = random_topologies(4, 8, seed=7)
    w = int_weights(4, 120, seed=3)
    w[1, -1] = 3.0  # per-tree weights, no outlier: the climb should be about the data
    res = nni_hill_climb(ch, lv, cost, weights=w, device=device)
    assert res.n_moves.sum() >= 1
    assert np.array_equal(res.scores, weighted_forward(device, res.children, lv, cost, w))
    for b in range(4):
        ref_ch, ref_h = R.greedy_ref(ch[b], expand(lv, w[b], 1), cost, 0.0, 1e-5)
        assert res.history[b] == ref_h, (b, res.history[b], ref_h)
        assert np.array_equal(res.children[b], ref_ch)
    shared = nni_hill_climb(ch, lv, cost, weights=w[0], device=device)  # (L,): every tree
    assert np.array_equal(shared.children[0], res.children[0])
    assert shared.history[0] == res.history[0]
    ref_ch, ref_h = R.greedy_ref(ch[2], expand(lv, w[0], 1), cost, 0.0, 1e-5)
    assert shared.history[2] == ref_h and np.array_equal(shared.children[2], ref_ch)


def test_stepwise_addition_equals_itself_on_the_expanded_alignment(device):
    lv = alignment()
    cost = general_cost(4, 1, "asym_int")
    w = int_weights(2, 120, seed=4)[0]
    rng = np.random.default_rng(5)
    order = np.stack([np.arange(8), np.arange(8)[::-1], rng.permutation(8), rng.permutation(8)])
    got = stepwise_addition(lv, cost, order=order, weights=w, device=device)
    want = stepwise_addition(expand(lv, w, 1), cost, order=order, device=device)
    plain = stepwise_addition(lv, cost, order=order, device=device)
    assert np.array_equal(got.children, want.children)
    assert np.array_equal(got.scores, want.scores)
    assert not np.array_equal(got.scores, plain.scores)
    per_tree = stepwise_addition(lv, cost, order=order, weights=np.tile(w, (4, 1)), device=device)
    assert np.array_equal(per_tree.children, got.children)


def test_parsimony_search_on_patterns_equals_the_full_alignment(device):
    lv = alignment()
    cost = general_cost(4, 1, "asym_int")
    patterns, counts, _ = compress_sites(lv)
    got = parsimony_search(patterns, cost, n_trees=4, seed=3, weights=counts, device=device)
    want = parsimony_search(lv, cost, n_trees=4, seed=3, device=device)
    assert np.array_equal(got.children, want.children)
    assert np.array_equal(got.scores, want.scores)
    assert np.array_equal(got.start_scores, want.start_scores)
    assert got.history == want.history and got.rounds == want.rounds
    assert np.array_equal(got.n_moves, want.n_moves) and np.array_equal(got.order, want.order)


def test_ratchet_equals_a_reference_loop(device):
    n_iter, frac, seed, min_gain = 3, 0.25, 2, 1e-5
    lv = alignment()
    cost = general_cost(4, 1, "asym_int")
    ch = random_topologies(4, 8, seed=7)
    w = int_weights(4, 120, seed=6)
    w[1, -1] = 2.0
    res = parsimony_ratchet(ch, lv, cost, weights=w, n_iter=n_iter, frac=frac, seed=seed,
                            min_gain=min_gain, device=device)

    def climb(tree, wb):
        return R.greedy_ref(tree, expand(lv, wb, 1), cost, 0.0, min_gain)

    rng = np.random.default_rng(seed)
    cur, best, best_ch, hist = [], [], [], []
    for b in range(4):
        t, h = climb(ch[b], w[b])
        cur.append(t), best.append(h[-1]), best_ch.append(t), hist.append([h[-1]])
    improved = np.zeros(4, dtype=np.int64)
    for _ in range(n_iter):
        mask = rng.random((4, 120)) < frac
        for b in range(4):
            up, _ = climb(cur[b], w[b] * (1 + mask[b]))
            cur[b], h = climb(up, w[b])
            if h[-1] < best[b]:
                best[b], best_ch[b] = h[-1], cur[b]
                improved[b] += 1
            hist[b].append(best[b])
    assert res.history == hist, (res.history, hist)
    assert np.array_equal(res.children, np.stack(best_ch))
    assert np.array_equal(res.n_improved, improved)
    for h in res.history:
        assert len(h) == n_iter + 1 and all(y <= x for x, y in zip(h, h[1:])), h
    assert res.scores.dtype == np.float32 and [h[-1] for h in res.history] == list(res.scores)
    fwd = np.array([weighted_forward(device, res.children[b:b + 1], lv, cost, w[b])[0]
                    for b in range(4)])
    assert np.array_equal(res.scores, fwd)
    # weights=None is all ones
    r1 = parsimony_ratchet(ch, lv, cost, n_iter=1, seed=seed, device=device)
    r2 = parsimony_ratchet(ch, lv, cost, weights=np.ones(120), n_iter=1, seed=seed, device=device)
    assert r1.history == r2.history and np.array_equal(r1.children, r2.children)


def test_bootstrap_search(device):
    min_gain = 1e-5
    lv = alignment()
    cost = general_cost(4, 1, "asym_int")
    res = bootstrap_search(lv, cost, n_replicates=4, seed=8, device=device)
    w = res.weights
    assert np.array_equal(w, bootstrap_weights(np.ones(120), 4, seed=8))
    assert w.shape == (4, 120) and (w.sum(axis=1) == 120).all() and (w == 0).any()
    s = res.search
    assert s.children.shape == (4, 15, 2)
    fwd = np.array([weighted_forward(device, s.children[b:b + 1], lv, cost, w[b])[0]
                    for b in range(4)])
    assert np.array_equal(s.scores, fwd)
    # a local optimum under the replicate's own weights, by the engine's forward
    moves = [(v, k) for v in range(8, 14) for k in (0, 1)]
    for b in range(4):
        nb = np.stack([apply_nni(s.children[b], v, k) for v, k in moves])
        nts = weighted_forward(device, nb, lv, cost, w[b]).astype(np.float64)
        assert (nts >= float(s.scores[b]) - min_gain * abs(float(s.scores[b]))).all(), b
    ref = parsimony_search(lv, cost, n_trees=1, device=device).children[0]
    sup = clade_support(ref, s.children)
    assert sup.shape == (7,) and (sup >= 0).all() and (sup <= 1).all() and sup[-1] == 1.0
    # compressed: the same replicates drawn over the patterns' counts
    patterns, counts, _ = compress_sites(lv)
    rc = bootstrap_search(patterns, cost, n_replicates=4, weights=counts, seed=8, device=device)
    assert rc.weights.shape == (4, 44) and (rc.weights.sum(axis=1) == 120).all()


# ---------------------------------------------------------------------------
# 9. guard bands
# ---------------------------------------------------------------------------
def g_weighted_sum(run, site_score, w):
    check, lib, ptr, st = G._abi(run.device)
    nb, L = w.shape
    ss, wt = run.input("site_score", site_score), run.input("weights", w)
    ts = run.output("tree_score", (nb,), G.F32)
    check(lib.trex_site_weighted_sum(ptr(ss), ptr(wt), nb, L, ptr(ts), st))


def g_nni_w(run, plan, leaves, cost, L, Q, tau, dp, outside, w):
    check, lib, ptr, st = G._abi(run.device)
    pl, lv, c = run.input("nni_plan", plan.nni_host), run.input("leaves", leaves), \
        run.input("cost", cost)
    dpt, ot, wt = run.input("dp", dp), run.input("outside", outside), run.input("weights", w)
    score = run.output("nni_score", (plan.B, plan.n_int - 1, 2), G.F32)
    nb = int(lib.trex_nni_workspace_bytes(plan.B, L, plan.n_all, Q))
    ws = run.workspace(nb)
    check(lib.trex_sankoff_nni_w(ptr(pl), ptr(lv), ptr(c), plan.B, L, plan.n_all, Q, float(tau),
                                 ptr(dpt), ptr(ot), ptr(wt), ptr(score), ptr(ws), nb, st))


def g_attach_w(run, plan, leaves, cost, L, Q, tau, dp, outside, w, *, new_leaf=None,
               sub_rows=None):
    check, lib, ptr, st = G._abi(run.device)
    pl, lv, c = run.input("attach_plan", plan.attach_host), run.input("leaves", leaves), \
        run.input("cost", cost)
    dpt, ot, wt = run.input("dp", dp), run.input("outside", outside), run.input("weights", w)
    nl, sr = run.input("new_leaf", new_leaf), run.input("sub_rows", sub_rows)
    score = run.output("attach_score", (plan.B, plan.n_all), G.F32)
    nb = int(lib.trex_attach_workspace_bytes(plan.B, L, plan.n_all, Q))
    ws = run.workspace(nb)
    check(lib.trex_sankoff_attach_w(ptr(pl), ptr(lv), ptr(c), plan.B, L, plan.n_all, Q,
                                    float(tau), ptr(dpt), ptr(ot), ptr(nl), ptr(sr), ptr(wt),
                                    ptr(score), ptr(ws), nb, st))


@pytest.mark.parametrize("tau", [0.0, 0.5])
@pytest.mark.parametrize("n,L,Q", [(6, 70, 4), (8, 65, 20)])
def test_guard_bands(device, n, L, Q, tau):
    """R0 / R1 / R2 of tests/_guard.py on the three entry points.  R2's input
    guard is 0xFF: a NaN weight directly behind the [B][L] payload."""
    ch = random_topologies(B, n, seed=7 * n + L)
    leaves = random_leaves(B, n, L, Q, seed=100 * Q + L + n, missing=0.05)
    cost = general_cost(Q, 1, "asym_frac" if tau else "asym_int")
    w = frac_weights(B, L, seed=n)
    new_leaf = random_leaves(B, 1, L, Q, seed=Q + L, missing=0.05)[:, 0]
    plan = TreePlan(ch)
    eng = SankoffEngine(plan, L, Q, device)
    lv, c, wd = dev(leaves, device), dev(cost, device), dev(w, device)
    f = eng.forward(lv, c, tau, site_score=True)
    out_dev = eng.outside(lv, c, tau, f.dp)
    dp, outside, ss = f.dp.cpu(), out_dev.cpu(), f.site_score.cpu()
    sub_rows = np.ascontiguousarray(dp.numpy()[:, -1])
    G.protocol(device, lambda: dict(tree_score=eng.weighted_score(f.site_score, wd)),
               lambda run: g_weighted_sum(run, ss, w))
    G.protocol(device,
               lambda: dict(nni_score=eng.nni_scores(lv, c, tau, dp=f.dp, outside=out_dev,
                                                     weights=wd)),
               lambda run: g_nni_w(run, plan, leaves, cost, L, Q, tau, dp, outside, w))
    G.protocol(device, lambda: dict(attach_score=eng.attach_scores(
        lv, c, tau, new_leaf=dev(new_leaf, device), dp=f.dp, outside=out_dev, weights=wd)),
        lambda run: g_attach_w(run, plan, leaves, cost, L, Q, tau, dp, outside, w,
                               new_leaf=new_leaf))
    G.protocol(device, lambda: dict(attach_score=eng.attach_scores(
        lv, c, tau, sub_rows=dev(sub_rows, device), dp=f.dp, outside=out_dev, weights=wd)),
        lambda run: g_attach_w(run, plan, leaves, cost, L, Q, tau, dp, outside, w,
                               sub_rows=sub_rows))


# ---------------------------------------------------------------------------
# 10. refusals
# ---------------------------------------------------------------------------
def test_bad_weights_are_refused(device):
    n, L, Q = 5, 8, 4
    eng = SankoffEngine(TreePlan(random_topologies(2, n, seed=0)), L, Q, device)
    lv = dev(random_leaves(2, n, L, Q, seed=1), device)
    c = dev(general_cost(Q, 2, "asym_int"), device)
    new = lv[:, 0].contiguous()
    f = eng.forward(lv, c, 0.0, site_score=True)
    good = torch.ones((2, L), dtype=torch.float32, device=device)
    bad = [good.double(), good.to(torch.int32), good[:, :7].contiguous(), good[0].contiguous(),
           good[:1].contiguous(), torch.ones((L, 2), dtype=torch.float32, device=device).t(),
           good.cpu(), good.cpu().numpy()]
    assert bad[5].shape == good.shape and not bad[5].is_contiguous()
    for w in bad:
        with pytest.raises(ValueError):
            eng.forward(lv, c, 0.0, weights=w)
        with pytest.raises(ValueError):
            eng.weighted_score(f.site_score, w)
        with pytest.raises(ValueError):
            eng.nni_scores(lv, c, 0.0, dp=f.dp, weights=w)
        with pytest.raises(ValueError):
            eng.attach_scores(lv, c, 0.0, new_leaf=new, dp=f.dp, weights=w)
    for ss in (f.site_score.double(), f.site_score[:, :7].contiguous(), f.site_score.cpu()):
        with pytest.raises(ValueError):
            eng.weighted_score(ss, good)
    with pytest.raises(ValueError):
        eng.weighted_score(f.site_score, good, out=torch.empty(3, device=device))
    assert torch.equal(eng.forward(lv, c, 0.0, weights=good).tree_score, f.tree_score)
