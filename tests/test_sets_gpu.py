"""GPU tests of state-set leaves (sankoff_sets.hip, sankoff_rows.h): int32
masks through forward, outside, nni_scores, attach_scores, backtrack and the
search functions, against the int8 code path (singleton masks: bitwise at
tau = 0) and the fp64 brute-force reference of _sets_ref.py.

Shapes (n_leaves, L, Q), B = 3 with a different topology per tree: L = 1 (one
lane), 64 (a full wave), 65 (tail lanes), 130 (three tiles of partial sums);
3 leaves (the minimum), a 5-leaf caterpillar (a chain of rows the lane wrote
itself), the 8-leaf balanced tree; Q = 2, 3, 4 (the register instantiations),
5 and 20 (both ends of the padded path).

Bars.  tau = 0 with integer costs: exact.  Otherwise relative
``max(1e-5, cond_rtol(dmax, tau))`` per tree as in tests/test_nni_gpu.py,
with dmax the largest |D| of the tree's internal rows in the fp64 reference
(an empty mask puts 1e5 into them; a leaf's own 1e5 entries never reach a
sum: their weights underflow to exactly 0).  A site's score is compared with
the absolute bound bar_l * d_l, d_l the largest internal |D| of that site and
bar_l the same formula on d_l (so 1e-5 on every site without an empty mask):
the score is a combination of such D values, each rounded at its own
magnitude, and a softmin score may itself be near zero.
"""

from __future__ import annotations

import functools
import itertools
import math

import numpy as np
import pytest
import torch

import _nni_ref as R
import _sets_ref as S
from _cases import (balanced_children, cond_rtol, general_cost, int_cost, random_leaves,
                    random_topologies)
from trex_amd import (SankoffEngine, TreePlan, TrexError, compress_sites, nni_hill_climb,
                      parsimony_search, sets_from_codes, stepwise_addition)
from trex_amd._lib import TREX_E_UNSUPPORTED

pytestmark = pytest.mark.gpu

B = 3
SHAPES = [(3, 1, 2), (5, 64, 3), (8, 65, 4), (8, 130, 5), (5, 65, 20)]
IDS = [f"n{n}-L{L}-q{Q}" for n, L, Q in SHAPES]


def caterpillar(n):
    ch = np.full((2 * n - 1, 2), -1, dtype=np.int32)
    ch[n] = (0, 1)
    for k in range(1, n - 1):
        ch[n + k] = (k + 1, n + k - 1)
    return ch


@functools.lru_cache(maxsize=None)
def topologies(n):
    ch = random_topologies(B, n, seed=31 * n)
    if n >= 5:
        ch[1] = caterpillar(n)
    if n == 8:
        ch[0] = balanced_children(8)[0]
    ch.setflags(write=False)
    return ch


def mixed_masks(shape, Q, seed, empty=True):
    """Per cell: 60 % one state, 25 % two or three, 10 % all, 5 % none
    (empty=False: those get one state)."""
    rng = np.random.default_rng(seed)
    u = rng.random(shape)
    out = np.zeros(shape, dtype=np.int64)
    for idx in np.ndindex(*shape):
        if u[idx] < 0.60 or (u[idx] >= 0.95 and not empty):
            out[idx] = 1 << int(rng.integers(Q))
        elif u[idx] < 0.85:
            k = min(Q, int(rng.integers(2, 4)))
            out[idx] = sum(1 << int(s) for s in rng.choice(Q, size=k, replace=False))
        elif u[idx] < 0.95:
            out[idx] = (1 << Q) - 1
    return out.astype(np.int32)


def cost_of(Q, tau, kind):
    if kind == "int":
        return int_cost(Q, seed=Q)
    return general_cost(Q, Q, "asym_int" if kind == "asym_int" else "asym_frac")


@functools.lru_cache(maxsize=None)
def case(n, L, Q, tau, masks="mixed", kind=None):
    """Host inputs and the fp64 references of one case, computed once and
    shared (read-only).  masks: "mixed" or "single" (sets_from_codes of
    random_leaves with 10 % missing; the codes are returned too)."""
    ch = topologies(n)
    kind = kind or ("asym_int" if tau == 0.0 else "asym_frac")
    cost = cost_of(Q, tau, kind).astype(np.float32)
    codes = new_codes = None
    if masks == "single":
        allc = random_leaves(B, n + 1, L, Q, seed=n + L + Q, missing=0.1)
        codes, new_codes = np.ascontiguousarray(allc[:, :n]), np.ascontiguousarray(allc[:, n])
        m, new = sets_from_codes(codes, Q), sets_from_codes(new_codes, Q)
    else:
        allm = mixed_masks((B, n + 1, L), Q, seed=n + L + Q)
        m, new = np.ascontiguousarray(allm[:, :n]), np.ascontiguousarray(allm[:, n])
    w = np.random.default_rng(n + L).uniform(0.25, 2.0, size=(B, L)).astype(np.float32)
    # a subtree's inside rows: integers where the case is compared exactly
    rs = np.random.default_rng(Q + L)
    sub = (rs.integers(0, 4, size=(B, L, Q)) if tau == 0.0 else
           rs.uniform(0.0, 3.0, size=(B, L, Q))).astype(np.float32)
    rows, new_rows = S.rows_from_masks(m, Q), S.rows_from_masks(new, Q)
    ref = []
    for b in range(B):
        r = dict(fwd=S.forward_ref(ch[b], rows[b], cost, tau),
                 hard=S.forward_ref(ch[b], rows[b], cost, tau, hard_root=True),
                 fwd_w=S.forward_ref(ch[b], rows[b], cost, tau, weights=w[b]),
                 attach=S.attach_ref(ch[b], rows[b], cost, tau, new_rows[b]),
                 attach_w=S.attach_ref(ch[b], rows[b], cost, tau, new_rows[b], weights=w[b]),
                 attach_sub=S.attach_ref(ch[b], rows[b], cost, tau, sub[b]),
                 nni=S.nni_ref(ch[b], rows[b], cost, tau),
                 nni_w=S.nni_ref(ch[b], rows[b], cost, tau, weights=w[b]))
        ref.append(r)
    return dict(ch=ch, cost=cost, masks=m, new=new, codes=codes, new_codes=new_codes, w=w,
                sub=sub, ref=ref, n=n, L=L, Q=Q, tau=tau)


def dev(x, device):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device)


def run(device, c, leaves, new_leaf, hard_root=False):
    """Every pass on one leaf encoding -> dict of device tensors."""
    n, L, Q, tau = c["n"], c["L"], c["Q"], c["tau"]
    eng = SankoffEngine(TreePlan(np.array(c["ch"])), L, Q, device)
    lv, nl, cd, w = dev(leaves, device), dev(new_leaf, device), dev(c["cost"], device), \
        dev(c["w"], device)
    sub = dev(c["sub"], device)
    f = eng.forward(lv, cd, tau, site_score=True)
    out = dict(eng=eng, lv=lv, cd=cd, dp=f.dp, site_score=f.site_score, tree_score=f.tree_score)
    fh = eng.forward(lv, cd, tau, site_score=True, hard_root=True)
    out["hard_site"], out["hard_tree"] = fh.site_score, fh.tree_score
    out["tree_w"] = eng.forward(lv, cd, tau, weights=w).tree_score
    out["outside"] = o = eng.outside(lv, cd, tau, f.dp)
    kw = dict(dp=f.dp, outside=o)
    out["nni"] = eng.nni_scores(lv, cd, tau, **kw)
    out["nni_w"] = eng.nni_scores(lv, cd, tau, weights=w, **kw)
    out["attach"] = eng.attach_scores(lv, cd, tau, new_leaf=nl, **kw)
    out["attach_w"] = eng.attach_scores(lv, cd, tau, new_leaf=nl, weights=w, **kw)
    out["attach_sub"] = eng.attach_scores(lv, cd, tau, sub_rows=sub, **kw)
    torch.cuda.synchronize()
    return out


OUTPUTS = ("dp", "site_score", "tree_score", "hard_site", "hard_tree", "tree_w", "outside", "nni",
           "nni_w", "attach", "attach_w", "attach_sub")


def assert_same_bits(a, b, names=OUTPUTS, skip=()):
    for k in names:
        if k not in skip:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def check_against_ref(c, got):
    """Every output of ``run`` against the fp64 reference of the case."""
    n, L, Q, tau, ref = c["n"], c["L"], c["Q"], c["tau"], c["ref"]
    nl = n
    exact = tau == 0.0
    g = {k: got[k].cpu().numpy().astype(np.float64) for k in OUTPUTS}
    worst = {}
    for b in range(B):
        D = ref[b]["fwd"]["inside"][nl:]  # (n_int, L, Q)
        dsite = np.abs(D).max(axis=(0, 2))  # (L,)
        bar = 1e-5 if exact else max(1e-5, cond_rtol(np.array([dsite.max()]), tau))
        # per site: only a site that has an empty mask in it carries the 1e5 offsets
        bar_l = 1e-5 if exact else np.maximum(1e-5, 2.0 * 2.0 ** -24 * dsite / tau)

        def rel(name, x, y):
            if exact:
                assert np.array_equal(x, np.asarray(y, np.float64).astype(np.float32)), (name, b)
                return
            e = float((np.abs(x - y) / np.abs(y)).max())
            worst[name] = max(worst.get(name, 0.0), e / bar)
            assert e <= bar, f"{name} tree {b}: rel err {e:.3e} > {bar:.3e}"

        def site(name, x, y):
            if exact:
                assert np.array_equal(x, np.broadcast_to(y, x.shape).astype(np.float32)), (name, b)
                return
            e = float((np.abs(x - y) / (bar_l * dsite)).max())
            worst[name] = max(worst.get(name, 0.0), e)
            assert e <= 1.0, f"{name} tree {b}: err / bound {e:.3e}"

        site("site_score", g["site_score"][b], ref[b]["fwd"]["site_score"])
        site("hard_site", g["hard_site"][b], ref[b]["hard"]["site_score"])
        # outside rows through the invariant (+)_i (O_v + D_v) = site score at every internal v
        inv = R.oplus(g["outside"][b] + g["dp"][b], tau)  # (n_int, L)
        site("invariant", inv, ref[b]["fwd"]["site_score"][None, :])
        assert not g["outside"][b, -1].any(), "root outside row is zeros"
        if exact:
            assert np.array_equal(g["dp"][b], D.astype(np.float32)), ("dp", b)
        rel("tree_score", g["tree_score"][b], ref[b]["fwd"]["tree_score"])
        rel("hard_tree", g["hard_tree"][b], ref[b]["hard"]["tree_score"])
        rel("attach", g["attach"][b], ref[b]["attach"])
        rel("attach_sub", g["attach_sub"][b], ref[b]["attach_sub"])
        rel("nni", g["nni"][b], ref[b]["nni"])
        # weighted: fractional weights, so never exact
        exact_was, exact = exact, False
        rel("tree_w", g["tree_w"][b], ref[b]["fwd_w"]["tree_score"])
        rel("attach_w", g["attach_w"][b], ref[b]["attach_w"])
        rel("nni_w", g["nni_w"][b], ref[b]["nni_w"])
        exact = exact_was
    print(f"n={n} L={L} Q={Q} tau={tau}: worst err / bar " +
          ", ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))


# 1. singleton masks are the code path -----------------------------------------
@pytest.mark.parametrize("kind", ["int", "frac"])
@pytest.mark.parametrize("n,L,Q", SHAPES, ids=IDS)
def test_singletons_equal_the_code_path_bitwise_at_tau0(device, n, L, Q, kind):
    c = case(n, L, Q, 0.0, "single", kind)
    a = run(device, c, c["masks"], c["new"])
    b = run(device, c, c["codes"], c["new_codes"])
    # the reduction tree of tree_score differs from the code forward's: exact
    # sums (integer costs) agree bitwise, others with the rounded exact sum
    general = ("tree_score", "hard_tree") if kind == "frac" else ()
    assert_same_bits(a, b, skip=general)
    for ts, ss in (("tree_score", "site_score"), ("hard_tree", "hard_site")):
        got = a[ts].cpu().numpy()
        want = np.array([np.float32(math.fsum(row)) for row in a[ss].cpu().numpy().tolist()],
                        dtype=np.float32)
        ulp = np.abs(np.spacing(want))
        assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all(), ts
        if kind == "int":
            assert np.array_equal(got, want)


@pytest.mark.parametrize("n,L,Q", SHAPES, ids=IDS)
def test_singletons_softmin_within_the_bar(device, n, L, Q):
    c = case(n, L, Q, 0.5, "single")
    check_against_ref(c, run(device, c, c["masks"], c["new"]))


# 2. mixed masks against the fp64 reference --------------------------------------
@pytest.mark.parametrize("tau", [0.0, 0.5])
@pytest.mark.parametrize("n,L,Q", SHAPES, ids=IDS)
def test_mixed_masks_against_fp64_reference(device, n, L, Q, tau):
    c = case(n, L, Q, tau)
    m = c["masks"]
    full = (1 << Q) - 1
    if L > 1:
        assert (m == 0).any() and (m == full).any()
    assert ((m & (m - 1)) != 0).any(), "no ambiguous cell"
    check_against_ref(c, run(device, c, m, c["new"]))


def test_repeated_calls_are_bitwise_equal(device):
    c = case(8, 130, 5, 0.5)
    a = run(device, c, c["masks"], c["new"])
    b = run(device, c, c["masks"], c["new"])
    assert_same_bits(a, b)


# 3. tau = 0: the minimum over the resolutions ---------------------------------
def test_tau0_site_score_is_the_minimum_over_resolutions(device):
    n, L, Q = 4, 65, 4
    rng = np.random.default_rng(5)
    masks = mixed_masks((n, L), Q, seed=5, empty=False)
    for l in range(L):  # at most three ambiguous leaves: at most 4^3 = 64 resolutions
        amb = np.flatnonzero((masks[:, l] & (masks[:, l] - 1)) != 0)
        if amb.size > 3:
            masks[amb[3:], l] = 1 << int(rng.integers(Q))
    assert (masks != 0).all() and ((masks & (masks - 1)) != 0).sum() > L // 2
    res = np.zeros((64, n, L), dtype=np.int8)
    most = 0
    for l in range(L):
        allowed = [[s for s in range(Q) if masks[x, l] >> s & 1] for x in range(n)]
        picks = list(itertools.product(*allowed))
        most = max(most, len(picks))
        assert len(picks) <= 64
        for r in range(64):
            res[r, :, l] = picks[r] if r < len(picks) else picks[0]
    assert most >= 16
    ch = random_topologies(1, n, seed=5)
    cost = general_cost(Q, 5, "asym_frac")
    cd = dev(cost, device)
    codes = SankoffEngine(TreePlan(np.repeat(ch, 64, axis=0)), L, Q, device).forward(
        dev(res, device), cd, 0.0, site_score=True).site_score
    sets = SankoffEngine(TreePlan(ch), L, Q, device).forward(
        dev(masks[None], device), cd, 0.0, site_score=True).site_score
    want = codes.min(dim=0).values
    assert torch.equal(sets[0].view(torch.int32), want.view(torch.int32))
    assert (codes.max(dim=0).values > want).any()  # the resolutions do differ


# 4. bits at or above Q ----------------------------------------------------------
@pytest.mark.parametrize("tau", [0.0, 0.5])
@pytest.mark.parametrize("n,L,Q", SHAPES, ids=IDS)
def test_high_bits_are_ignored(device, n, L, Q, tau):
    c = case(n, L, Q, tau)
    rng = np.random.default_rng(9)

    def dirty(m):
        hi = rng.integers(0, 1 << 11, size=m.shape).astype(np.int32) << 20  # bits 20 .. 30
        return m | hi

    m2, new2 = dirty(c["masks"]), dirty(c["new"])
    assert (m2 != c["masks"]).mean() > 0.9
    assert_same_bits(run(device, c, c["masks"], c["new"]), run(device, c, m2, new2))


# 5. weights -------------------------------------------------------------------
@pytest.mark.parametrize("tau", [0.0, 0.5])
def test_all_ones_weights_are_the_unweighted_bits(device, tau):
    c = dict(case(8, 130, 5, tau))
    c["w"] = np.ones_like(c["w"])
    a = run(device, c, c["masks"], c["new"])
    for plain, weighted in (("tree_score", "tree_w"), ("nni", "nni_w"), ("attach", "attach_w")):
        assert torch.equal(a[plain].view(torch.int32), a[weighted].view(torch.int32)), plain


# 6. backtrack -----------------------------------------------------------------
@pytest.mark.parametrize("n,L,Q", [(8, 65, 4), (5, 65, 20)], ids=["n8-q4", "n5-q20"])
def test_backtrack_states_add_up_to_the_site_score(device, n, L, Q):
    ch = topologies(n)
    masks = mixed_masks((B, n, L), Q, seed=77, empty=False)
    cost = int_cost(Q, seed=3)
    eng = SankoffEngine(TreePlan(np.array(ch)), L, Q, device)
    cd = dev(cost, device)
    f = eng.forward(dev(masks, device), cd, 0.0, site_score=True)
    anc = eng.backtrack(cd, f.dp).cpu().numpy()  # (B, n_int, L)
    site = f.site_score.cpu().numpy()
    for b in range(B):
        total = np.zeros(L)
        for node in range(n, 2 * n - 1):
            p = anc[b, node - n].astype(np.int64)  # (L,)
            assert ((p >= 0) & (p < Q)).all()
            for child in ch[b, node]:
                if child >= n:
                    s = anc[b, child - n].astype(np.int64)
                else:  # the first argmin over the leaf's set of C[parent state][s]
                    allowed = (masks[b, child][:, None] >> np.arange(Q)) & 1  # (L, Q)
                    s = np.where(allowed == 1, cost[p], np.inf).argmin(axis=1)
                total += cost[p, s]
        assert np.array_equal(total.astype(np.float32), site[b]), b


# 7. search --------------------------------------------------------------------
def test_search_on_singleton_masks_is_the_search_on_codes(device):
    n, L, Q = 8, 65, 4
    codes = random_leaves(1, n, L, Q, seed=12)[0]
    masks = sets_from_codes(codes, Q)
    cost = int_cost(Q, seed=12)
    kw = dict(tau=0.0, device=device)
    a, b = stepwise_addition(masks, cost, n_trees=3, seed=1, **kw), \
        stepwise_addition(codes, cost, n_trees=3, seed=1, **kw)
    assert np.array_equal(a.children, b.children) and np.array_equal(a.scores, b.scores)
    assert np.array_equal(a.order, b.order)
    start = random_topologies(3, n, seed=13)
    a, b = nni_hill_climb(start, masks, cost, **kw), nni_hill_climb(start, codes, cost, **kw)
    assert np.array_equal(a.children, b.children) and np.array_equal(a.scores, b.scores)
    assert a.history == b.history and np.array_equal(a.n_moves, b.n_moves)
    assert a.n_moves.sum() > 0
    a, b = parsimony_search(masks, cost, n_trees=3, seed=2, **kw), \
        parsimony_search(codes, cost, n_trees=3, seed=2, **kw)
    assert np.array_equal(a.children, b.children) and np.array_equal(a.scores, b.scores)
    assert a.history == b.history and np.array_equal(a.order, b.order)
    assert np.array_equal(a.start_scores, b.start_scores)


def test_search_on_an_ambiguous_alignment(device):
    n, L, Q = 8, 65, 4
    rng = np.random.default_rng(14)
    from _cases import simulate_leaves

    codes = simulate_leaves(n, L, Q, 12, seed=14)[0][:n]
    masks = sets_from_codes(codes, Q)
    amb = rng.random(masks.shape) < 0.20
    extra = rng.integers(1, 1 << Q, size=masks.shape).astype(np.int32)
    masks = np.where(amb, masks | extra, masks).astype(np.int32)
    assert ((masks & (masks - 1)) != 0).mean() > 0.1
    cost = int_cost(Q, seed=14)
    rows = S.rows_from_masks(masks, Q)
    min_gain = 1e-5

    def ref_score(ch):
        return S.forward_ref(ch, rows, cost, 0.0)["tree_score"]

    sw = stepwise_addition(masks, cost, n_trees=3, seed=3, tau=0.0, device=device)
    for b in range(3):
        assert sw.scores[b] == np.float32(ref_score(sw.children[b]))
    start = random_topologies(3, n, seed=15)
    hc = nni_hill_climb(start, masks, cost, tau=0.0, min_gain=min_gain, device=device)
    ps = parsimony_search(masks, cost, n_trees=3, seed=4, tau=0.0, min_gain=min_gain,
                          device=device)
    assert hc.n_moves.sum() > 0
    for r in (hc, ps):
        for b in range(3):
            cur = ref_score(r.children[b])
            assert r.scores[b] == np.float32(cur)
            h = r.history[b]
            assert all(y < x for x, y in zip(h, h[1:])), h
            assert h[-1] == float(r.scores[b])
            nb = S.nni_ref(r.children[b], rows, cost, 0.0)
            assert not (nb < cur - min_gain * abs(cur)).any(), (b, cur, nb.min())


def test_compressed_masks_score_like_the_alignment(device):
    n, Q = 8, 4
    base = mixed_masks((n, 20), Q, seed=16)
    index = np.random.default_rng(16).integers(0, 20, size=130)
    masks = np.ascontiguousarray(base[:, index])
    pat, counts, idx = compress_sites(masks)
    assert pat.dtype == np.int32 and pat.shape[1] <= 20
    assert np.array_equal(pat[:, idx], masks)
    ch = topologies(n)[:1]
    cd = dev(int_cost(Q, seed=16), device)
    full = SankoffEngine(TreePlan(np.array(ch)), 130, Q, device).forward(
        dev(masks[None], device), cd, 0.0).tree_score
    comp = SankoffEngine(TreePlan(np.array(ch)), pat.shape[1], Q, device).forward(
        dev(pat[None], device), cd, 0.0, weights=dev(counts[None], device)).tree_score
    assert torch.equal(full.view(torch.int32), comp.view(torch.int32))


# 8. refusals --------------------------------------------------------------------
def test_refusals(device):
    n, L, Q = 5, 65, 4
    ch = np.array(topologies(n))
    eng = SankoffEngine(TreePlan(ch), L, Q, device)
    m = dev(mixed_masks((B, n, L), Q, seed=1), device)
    cd = dev(int_cost(Q, seed=1), device)
    f = eng.forward(m, cd, 0.5)
    with pytest.raises(ValueError, match="int32"):
        eng.backward(m, cd, 0.5, f.dp)
    with pytest.raises(ValueError, match="int32"):
        eng.fwd_bwd(m, cd, 0.5)
    with pytest.raises(ValueError, match="int32"):
        eng.value_and_grad(m, cd, 0.5)
    with pytest.raises(ValueError, match="int32"):
        eng.to_trex_layout(f.dp, m)
    with pytest.raises(ValueError, match="new_leaf"):
        eng.attach_scores(m, cd, 0.0, new_leaf=torch.zeros((B, L), dtype=torch.int8,
                                                           device=device))
    with pytest.raises(ValueError, match="new_leaf"):
        eng.attach_scores(m.to(torch.int8), cd, 0.0, new_leaf=m[:, 0].contiguous())
    with pytest.raises(ValueError):
        eng.forward(m.to(torch.int64), cd, 0.0)
    eng21 = SankoffEngine(TreePlan(ch), L, 21, device)
    c21 = dev(int_cost(21, seed=1), device)
    with pytest.raises(TrexError, match="not supported") as e:
        eng21.forward(m, c21, 0.0)
    assert e.value.code == TREX_E_UNSUPPORTED
