"""GPU tests of the SPR neighbour scores (sankoff_spr.hip) and the SPR hill
climb: every entry against the fp64 references of _spr_ref.py (hard mode with
integer costs: exact), against the engine's own forward on rebuilt trees, the
+inf mask, the two identities (entry (v, sibling(v)) is the tree's score; an
NNI move is two SPR entries), state sets, weights, reproducibility, refusals,
spr_hill_climb and ``moves="spr"``."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import _nni_ref as R
import _spr_ref as S
from _cases import balanced_children, cond_rtol, general_cost, int_cost, random_leaves, \
    random_topologies
from test_attach_gpu import _stepwise_data
from test_nni_gpu import SHAPES, caterpillar, case as nni_case
from test_sets_gpu import mixed_masks
from trex_amd import (SankoffEngine, TreePlan, TrexError, apply_spr, nni_hill_climb,
                      parsimony_search, sets_from_codes, spr_hill_climb, stepwise_addition)
from trex_amd._lib import TREX_E_TOPOLOGY, TREX_E_UNSUPPORTED

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(n, L, Q, tau, missing=None):
    """test_nni_gpu.case's inputs (B = 3, asymmetric costs with a non-zero
    diagonal, missing codes at n = 6 in hard mode) with the fp64 SPR
    references, computed once per case and shared (read-only)."""
    ch, lv, cost, nni = nni_case(n, L, Q, tau, missing)
    ref = np.stack([S.spr_ref(ch[b], lv[b], cost, tau) for b in range(3)])
    bf = np.stack([S.brute_force(ch[b], lv[b], cost, tau) for b in range(3)])
    ok = np.stack([S.valid_mask(ch[b]) for b in range(3)])
    return ch, lv, cost, nni, ref, bf, ok


def run(device, ch, lv, cost, tau, weights=None):
    eng = SankoffEngine(TreePlan(ch), lv.shape[2], cost.shape[0], device)
    lvd = torch.from_numpy(np.ascontiguousarray(lv)).to(device)
    cd = torch.from_numpy(cost).to(device)
    f = eng.forward(lvd, cd, tau)
    out = eng.outside(lvd, cd, tau, f.dp)
    spr = eng.spr_scores(lvd, cd, tau, dp=f.dp, outside=out, weights=weights)
    torch.cuda.synchronize()
    return eng, lvd, cd, f, out, spr


def identities(ch, spr, ts, nni):
    """(own, nni0, nni1): spr's entries (v, sibling(v)) next to the tree score
    broadcast, and the two SPR entries of every NNI move next to nni."""
    B, n_all = ch.shape[0], ch.shape[1]
    n = (n_all + 1) // 2
    own = np.stack([[spr[b, v, R.relatives(ch[b])[1][v]] for v in range(n_all - 1)]
                    for b in range(B)])
    e0, e1 = np.zeros_like(nni), np.zeros_like(nni)
    for b in range(B):
        for v, k, a, c in S.identity_pairs(ch[b]):
            e0[b, v - n, k], e1[b, v - n, k] = spr[(b,) + a], spr[(b,) + c]
    return own, np.broadcast_to(ts[:, None], own.shape), e0, e1


@pytest.mark.parametrize("n,L,Q", SHAPES)
def test_hard_mode_is_exact(device, n, L, Q):
    ch, lv, cost, _, ref, bf, ok = case(n, L, Q, 0.0)
    eng, lvd, cd, f, out, spr = run(device, ch, lv, cost, 0.0)
    assert spr.shape == (3, 2 * n - 2, 2 * n - 1) and spr.dtype == torch.float32
    assert float(ref[ok].max()) < 2 ** 24  # integers exact in fp32
    assert np.array_equal(ref, bf)
    got = spr.cpu().numpy()
    assert np.array_equal(np.isinf(got), ~ok), "+inf mask"
    assert (got[~ok] > 0).all()
    assert np.array_equal(got, ref.astype(np.float32)), "against spr_ref"
    assert np.array_equal(got, bf.astype(np.float32)), "against the brute force"
    nni = eng.nni_scores(lvd, cd, 0.0, dp=f.dp, outside=out).cpu().numpy()
    own, ts, e0, e1 = identities(ch, got, f.tree_score.cpu().numpy(), nni)
    assert np.array_equal(own, ts), "identity 1"
    assert np.array_equal(e0, nni) and np.array_equal(e1, nni), "identity 2"
    # spr_scores runs the forward and the outside pass itself when not given
    assert torch.equal(eng.spr_scores(lvd, cd, 0.0), spr)
    assert torch.equal(eng.spr_scores(lvd, cd, 0.0, dp=f.dp), spr)


@pytest.mark.parametrize("which", ["n12", "n8"])
def test_walk_corner_cases(device, which):
    """A caterpillar of 12 (a path of 10 changed inside rows), a balanced
    tree of 8 and random trees; L = 65: the second tile has one live lane."""
    L, Q = 65, 4
    if which == "n12":
        n = 12
        ch = random_topologies(3, n, seed=77)
        ch[0] = caterpillar(n)
    else:
        n = 8
        ch = random_topologies(2, n, seed=78)
        ch[0] = balanced_children(8)[0]
    lv = random_leaves(len(ch), n, L, Q, seed=n, missing=0.03)
    cost = general_cost(Q, 5, "asym_int")
    _, _, _, _, _, spr = run(device, ch, lv, cost, 0.0)
    ref = np.stack([S.spr_ref(ch[b], lv[b], cost, 0.0) for b in range(len(ch))])
    assert float(ref[np.isfinite(ref)].max()) < 2 ** 24
    assert np.array_equal(spr.cpu().numpy(), ref.astype(np.float32))


def test_hard_mode_equals_engine_forward_on_rebuilt_trees(device):
    B, n, L, Q = 4, 16, 130, 4
    ch = random_topologies(B, n, seed=31)
    lv = random_leaves(B, n, L, Q, seed=32)
    cost = int_cost(Q, seed=33)
    lvd = torch.from_numpy(lv).to(device)
    cd = torch.from_numpy(cost).to(device)
    spr = SankoffEngine(TreePlan(ch), L, Q, device).spr_scores(lvd, cd, 0.0)
    assert spr.shape == (B, 2 * n - 2, 2 * n - 1)
    ok = np.stack([S.valid_mask(ch[b]) for b in range(B)])
    finite = torch.isfinite(spr).cpu().numpy()
    assert np.array_equal(finite, ok)
    idx = np.argwhere(ok)
    nb = np.stack([apply_spr(ch[b], v, x) for b, v, x in idx])
    nb_lv = lvd[torch.from_numpy(idx[:, 0]).to(device)].contiguous()
    ts = SankoffEngine(TreePlan(nb), L, Q, device).forward(nb_lv, cd, 0.0).tree_score
    assert torch.equal(spr[torch.from_numpy(ok).to(device)], ts)
    assert len(torch.unique(ts)) > 10  # the moves do change the score


@pytest.mark.parametrize("n,L,Q", SHAPES)
def test_softmin_within_1e5_of_fp64_brute_force(device, n, L, Q):
    tau = 0.5
    ch, lv, cost, _, ref, bf, ok = case(n, L, Q, tau)
    eng, lvd, cd, f, out, spr = run(device, ch, lv, cost, tau)
    got = spr.cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isinf(got), ~ok), "+inf mask"
    rel = np.abs(got[ok] - bf[ok]) / np.abs(bf[ok])
    print(f"spr softmin ({n}, {L}, {Q}): worst rel err {rel.max():.3e}")
    assert rel.max() <= 1e-5, f"neighbour scores: worst rel err {rel.max():.3e}"
    nni = eng.nni_scores(lvd, cd, tau, dp=f.dp, outside=out).cpu().numpy().astype(np.float64)
    own, ts, e0, e1 = identities(ch, got, f.tree_score.cpu().numpy().astype(np.float64), nni)
    assert (np.abs(own - ts) / np.abs(ts)).max() <= 1e-5, "identity 1"
    assert (np.abs(e0 - nni) / np.abs(nni)).max() <= 1e-5, "identity 2"
    assert (np.abs(e1 - nni) / np.abs(nni)).max() <= 1e-5, "identity 2"


def test_softmin_with_missing_codes(device):
    """5 % missing codes under the softmin: every D carries trex's 1e5
    offsets, so the bar is max(1e-5, cond_rtol) as in test_attach_gpu; the
    fp64 reference alone meets it against the fp64 brute force, then the
    device does."""
    n, L, Q, tau = 6, 70, 4, 0.5
    ch, lv, cost, nni, ref, bf, ok = case(n, L, Q, tau, 0.05)
    assert (lv < 0).any()
    dmax = max(float(np.abs(r["inside"]).max()) for r in nni)
    bar = max(1e-5, cond_rtol(np.array([dmax]), tau))
    rel_ref = np.abs(ref[ok] - bf[ok]) / np.abs(bf[ok])
    assert rel_ref.max() <= bar, f"fp64 reference vs brute force: {rel_ref.max():.3e} > {bar:.3e}"
    _, _, _, _, _, spr = run(device, ch, lv, cost, tau)
    got = spr.cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isinf(got), ~ok)
    rel = np.abs(got[ok] - bf[ok]) / np.abs(bf[ok])
    print(f"spr softmin with missing codes: fp64 reference {rel_ref.max():.3e}, device "
          f"{rel.max():.3e}, bar {bar:.3e}")
    assert rel.max() <= bar, f"neighbour scores: worst rel err {rel.max():.3e} > {bar:.3e}"


@pytest.mark.parametrize("tau", [0.0, 0.5])
@pytest.mark.parametrize("n,L,Q", [(6, 70, 4), (7, 33, 5)])
def test_singleton_sets_give_the_bits_of_the_code_path(device, n, L, Q, tau):
    """The SPR pass on masks 1 << code gives the bits it gives on the codes,
    from the same DP table (the two forwards are different kernels, whose
    softmin tables agree within the bar, not bitwise; at tau = 0 they are
    equal and the pass also runs from the state-set forward's own table)."""
    ch, lv, cost, *_ = case(n, L, Q, tau)
    eng, lvd, cd, f, out, spr = run(device, ch, lv, cost, tau)
    masks = sets_from_codes(lv, Q)
    assert masks.dtype == np.int32
    md = torch.from_numpy(masks).to(device)
    assert torch.equal(eng.spr_scores(md, cd, tau, dp=f.dp), spr)
    assert torch.equal(eng.spr_scores(md, cd, tau, dp=f.dp, outside=out), spr)
    if tau == 0.0:
        assert torch.equal(eng.spr_scores(md, cd, tau), spr)


@pytest.mark.parametrize("n,L,Q", [(6, 70, 4), (7, 33, 5)])
def test_ambiguity_masks_are_exact_at_tau0(device, n, L, Q):
    ch, _, cost, *_ = case(n, L, Q, 0.0)
    masks = mixed_masks((3, n, L), Q, seed=n + Q)
    assert ((masks & (masks - 1)) != 0).any() and (masks == 0).any()
    ref = np.stack([S.spr_ref(ch[b], S.mask_rows(masks[b], Q), cost, 0.0) for b in range(3)])
    assert float(ref[np.isfinite(ref)].max()) < 2 ** 24
    _, _, _, _, _, got = run(device, ch, masks, cost, 0.0)
    assert np.array_equal(got.cpu().numpy(), ref.astype(np.float32))


@pytest.mark.parametrize("tau", [0.0, 0.5])
def test_all_ones_weights_are_the_unweighted_bits(device, tau):
    ch, lv, cost, *_ = case(9, 129, 4, tau)
    _, _, _, _, _, spr = run(device, ch, lv, cost, tau)
    ones = torch.ones((3, 129), dtype=torch.float32, device=device)
    _, _, _, _, _, got = run(device, ch, lv, cost, tau, weights=ones)
    assert torch.equal(got, spr)


def test_integer_weights_repeat_columns(device):
    n, L, Q = 6, 70, 4
    ch, lv, cost, *_ = case(n, L, Q, 0.0)
    w = np.random.default_rng(3).integers(0, 4, size=L)
    assert (w == 0).any() and (w > 1).any()
    wd = torch.from_numpy(np.broadcast_to(w.astype(np.float32), (3, L)).copy()).to(device)
    _, _, _, _, _, got = run(device, ch, lv, cost, 0.0, weights=wd)
    rep = np.ascontiguousarray(np.repeat(lv, w, axis=2))
    _, _, _, _, _, want = run(device, ch, rep, cost, 0.0)
    assert float(want[torch.isfinite(want)].max()) < 2 ** 24
    assert torch.equal(got, want)


@pytest.mark.parametrize("tau", [0.0, 0.5])
def test_repeated_calls_are_bitwise_equal(device, tau):
    ch, lv, cost, *_ = case(9, 129, 4, tau)
    eng, lvd, cd, f, out, spr = run(device, ch, lv, cost, tau)
    for _ in range(2):
        assert torch.equal(eng.spr_scores(lvd, cd, tau, dp=f.dp, outside=out), spr)
    assert torch.equal(eng.spr_scores(lvd, cd, tau), spr)
    # another engine, whose workspace is a fresh allocation
    eng2 = SankoffEngine(TreePlan(ch), 129, 4, device)
    eng2._spr_ws = torch.full((eng._spr_ws.numel(),), 0xFF, dtype=torch.uint8, device=device)
    assert torch.equal(eng2.spr_scores(lvd, cd, tau, dp=f.dp, outside=out), spr)


def test_refusals(device):
    ch = random_topologies(2, 4, seed=0)
    L = 8
    eng = SankoffEngine(TreePlan(ch), L, 21, device)
    lv = torch.from_numpy(random_leaves(2, 4, L, 21, seed=1)).to(device)
    c = torch.from_numpy(int_cost(21, seed=2)).to(device)
    with pytest.raises(TrexError) as e:
        eng.spr_scores(lv, c, 0.0)
    assert e.value.code == TREX_E_UNSUPPORTED
    # the C entry point itself, on tables of the right size
    from trex_amd._lib import lib, ptr, stream_handle

    tab = torch.zeros(eng.dp_shape, dtype=torch.float32, device=device)
    score = torch.zeros((2, 6, 7), dtype=torch.float32, device=device)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=device)
    for fn, leaves in ((lib().trex_sankoff_spr_w, lv),
                       (lib().trex_sankoff_sets_spr_w, lv.to(torch.int32))):
        rc = fn(ptr(eng.plan.spr_device(device)), ptr(leaves), ptr(c), 2, L, 7, 21, 0.0, ptr(tab),
                ptr(tab), None, ptr(score), ptr(ws), ws.numel(), stream_handle(device))
        assert rc == TREX_E_UNSUPPORTED
    assert lib().trex_spr_workspace_bytes(2, L, 7, 21) == 0

    two = np.array([[[-1, -1], [-1, -1], [0, 1]]], dtype=np.int32)
    eng2 = SankoffEngine(TreePlan(two), L, 4, device)
    lv2 = torch.from_numpy(random_leaves(1, 2, L, 4, seed=1)).to(device)
    c4 = torch.from_numpy(int_cost(4, seed=2)).to(device)
    with pytest.raises(TrexError) as e:
        eng2.spr_scores(lv2, c4, 0.0)
    assert e.value.code == TREX_E_TOPOLOGY
    rc = lib().trex_sankoff_spr_w(ptr(ws), ptr(lv2), ptr(c4), 1, L, 3, 4, 0.0, ptr(tab), ptr(tab),
                                  None, ptr(score), ptr(ws), ws.numel(), stream_handle(device))
    assert rc == TREX_E_TOPOLOGY

    eng = SankoffEngine(TreePlan(ch), L, 4, device)
    lv = torch.from_numpy(random_leaves(2, 4, L, 4, seed=1)).to(device)
    f = eng.forward(lv, c4, 0.0)
    out = eng.outside(lv, c4, 0.0, f.dp)
    w = torch.ones((2, L), dtype=torch.float32, device=device)
    with pytest.raises(ValueError):
        eng.spr_scores(lv[:, :, :4].contiguous(), c4, 0.0)
    with pytest.raises(ValueError):
        eng.spr_scores(lv.to(torch.int64), c4, 0.0)
    with pytest.raises(ValueError):
        eng.spr_scores(lv.cpu(), c4, 0.0)
    with pytest.raises(ValueError):
        eng.spr_scores(lv, c4[:3, :3].contiguous(), 0.0)
    with pytest.raises(ValueError):
        eng.spr_scores(lv, c4.double(), 0.0)
    with pytest.raises(ValueError):
        eng.spr_scores(lv, c4, 0.0, dp=f.dp[:, :2].contiguous())
    with pytest.raises(ValueError):
        eng.spr_scores(lv, c4, 0.0, dp=f.dp.transpose(2, 3))
    with pytest.raises(ValueError):
        eng.spr_scores(lv, c4, 0.0, dp=f.dp, outside=out.transpose(2, 3).contiguous())
    with pytest.raises(ValueError):
        eng.spr_scores(lv, c4, 0.0, outside=out)
    with pytest.raises(ValueError):
        eng.spr_scores(lv, c4, 0.0, dp=f.dp.double(), outside=out)
    with pytest.raises(ValueError):
        eng.spr_scores(lv, c4, 0.0, weights=w[:, :4])
    with pytest.raises(ValueError):
        eng.spr_scores(lv, c4, 0.0, weights=w.double())
    with pytest.raises(ValueError):
        eng.spr_scores(lv, c4, 0.0, weights=w.cpu())
    with pytest.raises(TrexError):
        eng.spr_scores(lv, c4, -1.0, dp=f.dp, outside=out)
    ws_small = torch.zeros(64, dtype=torch.uint8, device=device)
    rc = lib().trex_sankoff_spr_w(ptr(eng.plan.spr_device(device)), ptr(lv), ptr(c4), 2, L, 7, 4,
                                  0.0, ptr(f.dp), ptr(out), None, ptr(score), ptr(ws_small), 64,
                                  stream_handle(device))
    assert rc < 0


@pytest.mark.parametrize("Q,tau", [(4, 0.0), (4, 0.5), (20, 0.0)])
def test_spr_hill_climb(device, Q, tau):
    min_gain = 1e-5
    lv, cost, _ = _stepwise_data(Q)
    ch = random_topologies(4, 8, seed=7)
    res = spr_hill_climb(ch, lv, cost, tau=tau, device=device)
    assert res.children.shape == ch.shape and res.children.dtype == np.int32
    assert res.rounds == res.n_moves.max()
    cd = torch.from_numpy(cost).to(device)
    lvd = torch.from_numpy(lv).to(device)[None].expand(4, -1, -1).contiguous()
    TreePlan(res.children).spr_host  # proper trees
    ts = SankoffEngine(TreePlan(res.children), 120, Q, device).forward(lvd, cd, tau).tree_score
    assert np.array_equal(res.scores, ts.cpu().numpy())
    for b in range(4):
        h = res.history[b]
        assert all(y < x for x, y in zip(h, h[1:])), h
        assert len(h) == res.n_moves[b] + 1 and h[-1] == res.scores[b]
    assert res.n_moves.sum() >= 1
    if tau == 0.0:  # integer scores: the fp64 greedy takes the same path
        for b in range(4):
            ref_ch, ref_h = S.greedy_ref(ch[b], lv, cost, 0.0, min_gain)
            assert res.history[b] == ref_h, (b, res.history[b], ref_h)
            assert np.array_equal(res.children[b], ref_ch)
        # an SPR optimum is an NNI optimum
        again = nni_hill_climb(res.children, lv, cost, device=device)
        assert again.n_moves.sum() == 0 and np.array_equal(again.children, res.children)
        nni = nni_hill_climb(ch, lv, cost, device=device)
        print(f"Q={Q}: SPR {res.scores.tolist()} NNI {nni.scores.tolist()}")


@pytest.mark.parametrize("tau", [0.0, 0.5])
def test_parsimony_search_moves(device, tau):
    lv, cost, _ = _stepwise_data(4)
    res = parsimony_search(lv, cost, n_trees=4, seed=3, tau=tau, device=device, moves="spr")
    start = stepwise_addition(lv, cost, n_trees=4, seed=3, tau=tau, device=device)
    climb = spr_hill_climb(start.children, lv, cost, tau=tau, device=device)
    assert np.array_equal(res.start_scores, start.scores)
    assert np.array_equal(res.order, start.order)
    assert np.array_equal(res.children, climb.children)
    assert np.array_equal(res.scores, climb.scores)
    assert res.history == climb.history and res.rounds == climb.rounds
    assert np.array_equal(res.n_moves, climb.n_moves)
    plain = parsimony_search(lv, cost, n_trees=4, seed=3, tau=tau, device=device)
    named = parsimony_search(lv, cost, n_trees=4, seed=3, tau=tau, device=device, moves="nni")
    assert np.array_equal(plain.children, named.children)
    assert np.array_equal(plain.scores, named.scores)
    assert plain.history == named.history and plain.rounds == named.rounds
    assert np.array_equal(plain.n_moves, named.n_moves)
    with pytest.raises(ValueError):
        parsimony_search(lv, cost, n_trees=4, device=device, moves="x")
