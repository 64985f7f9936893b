"""GPU tests of the NNI neighbour scores (sankoff_nni.hip) and the hill climb:
outside table, invariant and move scores against the fp64 references of
_nni_ref.py (hard mode with integer costs: exact), against the engine's own
forward on rebuilt topologies, reproducibility, refusals, nni_hill_climb."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import _nni_ref as R
from _cases import (assert_cost_is_general, balanced_children, cond_rtol, general_cost, hamming,
                    int_cost, random_leaves, random_topologies, simulate_leaves)
from trex_amd import SankoffEngine, TreePlan, TrexError, apply_nni, nni_hill_climb
from trex_amd._lib import TREX_E_UNSUPPORTED

pytestmark = pytest.mark.gpu


def caterpillar(n):
    ch = np.full((2 * n - 1, 2), -1, dtype=np.int32)
    ch[n] = (0, 1)
    for k in range(1, n - 1):
        ch[n + k] = (k + 1, n + k - 1)
    return ch


# (n_leaves, L, Q): L straddles the wave size (64); n = 3 has the single
# non-root edge with all-leaf neighbours; Q = 5 and 20 take the padded path
SHAPES = [(3, 1, 2), (4, 63, 3), (6, 70, 4), (9, 129, 4), (7, 33, 5), (8, 65, 20)]


@functools.lru_cache(maxsize=None)
def case(n, L, Q, tau, missing=None):
    """Inputs (B = 3, a different topology per tree) and the fp64 references,
    computed once per case and shared (treated as read-only).  Costs are
    asymmetric with a non-zero diagonal (tests/_cases.py general_cost):
    integers for the hard cases, so their scores stay exact, uniform(0.25, 2)
    for the softmin ones; the oracle tells C from C^T on every case
    (assert_cost_is_general), so the DYN path's p[i * Q + j] and the TRANS
    messages cannot be read the other way round unnoticed."""
    ch = random_topologies(3, n, seed=10 * n + Q)
    if n == 8:
        ch[0] = balanced_children(8)[0]
        ch[1] = caterpillar(8)
    if n == 9:
        ch[1] = caterpillar(9)
    hard = tau == 0.0
    if missing is None:
        missing = 0.05 if (hard and n == 6) else 0.0
    lv = random_leaves(3, n, L, Q, seed=n + L, missing=missing)
    kind = "asym_int" if hard else "asym_frac"
    cost = general_cost(Q, Q, kind)
    assert_cost_is_general(cost, ch, lv, tau)
    ref = [R.nni_ref(ch[b], lv[b], cost, tau) for b in range(3)]
    return ch, lv, cost.astype(np.float32), ref


def run(device, ch, lv, cost, tau):
    eng = SankoffEngine(TreePlan(ch), lv.shape[2], cost.shape[0], device)
    lvd = torch.from_numpy(lv).to(device)
    cd = torch.from_numpy(cost).to(device)
    f = eng.forward(lvd, cd, tau, site_score=True)
    out = eng.outside(lvd, cd, tau, f.dp)
    nni = eng.nni_scores(lvd, cd, tau, dp=f.dp, outside=out)
    torch.cuda.synchronize()
    return eng, lvd, cd, f, out, nni


@pytest.mark.parametrize("n,L,Q", SHAPES)
def test_hard_mode_is_exact(device, n, L, Q):
    ch, lv, cost, ref = case(n, L, Q, 0.0)
    eng, lvd, cd, f, out, nni = run(device, ch, lv, cost, 0.0)
    ref_out = torch.from_numpy(np.stack([r["outside"] for r in ref]).astype(np.float32))
    ref_nni = torch.from_numpy(np.stack([r["nni"] for r in ref]).astype(np.float32))
    ref_ts = torch.from_numpy(np.array([r["tree_score"] for r in ref]).astype(np.float32))
    assert float(np.max([r["nni"].max() for r in ref])) < 2 ** 24  # integers exact in fp32
    assert nni.shape == (3, n - 2, 2) and nni.dtype == torch.float32
    assert torch.equal(f.tree_score.cpu(), ref_ts)
    assert torch.equal(out.cpu(), ref_out), "outside table"
    assert not out[:, -1].any(), "root row is zeros"
    # invariant: min_i (O_v[i] + D_v[i]) is the site score at every internal v
    inv = (out + f.dp).min(dim=-1).values  # (B, n_int, L)
    assert torch.equal(inv, f.site_score[:, None, :].expand_as(inv)), "invariant"
    assert torch.equal(nni.cpu(), ref_nni), "neighbour scores"
    # nni_scores runs the forward and the outside pass itself when not given
    assert torch.equal(eng.nni_scores(lvd, cd, 0.0), nni)
    assert torch.equal(eng.nni_scores(lvd, cd, 0.0, dp=f.dp), nni)


def test_hard_mode_equals_engine_forward_on_rebuilt_trees(device):
    B, n, L, Q = 64, 32, 300, 4
    ch = random_topologies(B, n, seed=21)
    lv = random_leaves(B, n, L, Q, seed=22)
    cost = int_cost(Q, seed=23)
    lvd = torch.from_numpy(lv).to(device)
    cd = torch.from_numpy(cost).to(device)
    nni = SankoffEngine(TreePlan(ch), L, Q, device).nni_scores(lvd, cd, 0.0)
    assert nni.shape == (B, n - 2, 2)
    moves = [(v, k) for v in range(n, 2 * n - 2) for k in (0, 1)]
    nb = np.stack([apply_nni(ch[b], v, k) for b in range(B) for v, k in moves])
    nb_lv = lvd.repeat_interleave(len(moves), dim=0).contiguous()
    ts = SankoffEngine(TreePlan(nb), L, Q, device).forward(nb_lv, cd, 0.0).tree_score
    assert torch.equal(nni.reshape(-1), ts)
    assert len(torch.unique(nni)) > 10  # the moves do change the score


# every instantiation: Q = 2, 3 (nni_*_kernel<2 | 3, false, true>), 4, the padded
# soft kernel with dead states (Q = 5: live(j) keeps them out of the exp-sum) and Q = 20
@pytest.mark.parametrize("n,L,Q", SHAPES)
def test_softmin_within_1e5_of_fp64_brute_force(device, n, L, Q):
    tau = 0.5
    ch, lv, cost, ref = case(n, L, Q, tau)
    eng, lvd, cd, f, out, nni = run(device, ch, lv, cost, tau)
    bf = np.stack([R.brute_force(ch[b], lv[b], cost, tau) for b in range(3)])
    got = nni.cpu().numpy().astype(np.float64)
    rel = np.abs(got - bf) / np.abs(bf)
    assert rel.max() <= 1e-5, f"neighbour scores: worst rel err {rel.max():.3e}"
    # invariant: sum over sites of smin_i (O_v[i] + D_v[i]) is the tree score
    o64 = out.cpu().numpy().astype(np.float64)
    d64 = f.dp.cpu().numpy().astype(np.float64)
    inv = R.oplus(o64 + d64, tau).sum(axis=-1)  # (B, n_int)
    ts = f.tree_score.cpu().numpy().astype(np.float64)
    rel_inv = np.abs(inv - ts[:, None]) / np.abs(ts[:, None])
    assert rel_inv.max() <= 1e-5, f"invariant: worst rel err {rel_inv.max():.3e}"
    ref_ts = np.array([r["tree_score"] for r in ref])
    rel_ts = np.abs(inv - ref_ts[:, None]) / np.abs(ref_ts[:, None])
    assert rel_ts.max() <= 1e-5, f"invariant vs fp64: worst rel err {rel_ts.max():.3e}"


def test_softmin_with_missing_codes(device):
    """5 % missing codes under the softmin: every D carries trex's 1e5
    offsets, so the bar is max(1e-5, cond_rtol) as in the wide kernels'
    missing-leaf tests; the fp64 outside-table reference alone meets it
    against the fp64 brute force, then the device does."""
    n, L, Q, tau = 6, 70, 4, 0.5
    ch, lv, cost, ref = case(n, L, Q, tau, 0.05)
    assert (lv < 0).any()
    bf = np.stack([R.brute_force(ch[b], lv[b], cost, tau) for b in range(3)])
    dmax = max(float(np.abs(r["inside"]).max()) for r in ref)
    bar = max(1e-5, cond_rtol(np.array([dmax]), tau))
    rel_ref = np.abs(np.stack([r["nni"] for r in ref]) - bf) / np.abs(bf)
    assert rel_ref.max() <= bar, f"fp64 reference vs brute force: {rel_ref.max():.3e} > {bar:.3e}"
    eng, lvd, cd, f, out, nni = run(device, ch, lv, cost, tau)
    rel = np.abs(nni.cpu().numpy().astype(np.float64) - bf) / np.abs(bf)
    print(f"nni softmin with missing codes: fp64 reference {rel_ref.max():.3e}, device "
          f"{rel.max():.3e}, bar {bar:.3e}")
    assert rel.max() <= bar, f"neighbour scores: worst rel err {rel.max():.3e} > {bar:.3e}"


@pytest.mark.parametrize("tau", [0.0, 0.5])
def test_repeated_calls_are_bitwise_equal(device, tau):
    ch, lv, cost, _ = case(9, 129, 4, tau)
    eng, lvd, cd, f, out, nni = run(device, ch, lv, cost, tau)
    for _ in range(2):
        assert torch.equal(eng.outside(lvd, cd, tau, f.dp), out)
        assert torch.equal(eng.nni_scores(lvd, cd, tau, dp=f.dp, outside=out), nni)


def test_scores_are_computed_from_the_callers_table(device):
    ch, lv, cost, _ = case(9, 129, 4, 0.0)
    eng, lvd, cd, f, out, nni = run(device, ch, lv, cost, 0.0)
    tab = eng.plan.nni_table  # (B, n_int - 1, 4): u, a0, a1, s
    nl = eng.plan.n_leaves
    tested = 0
    for r in range(eng.plan.n_int - 1):
        reads = (tab[0, :, 1:] == nl + r).any(axis=1)  # moves whose a0 / a1 / s is the row
        if not reads.any():
            continue
        dp2 = f.dp.clone()
        dp2[0, r] += 1.0
        got = eng.nni_scores(lvd, cd, 0.0, dp=dp2, outside=out)
        changed = (got != nni).any(dim=-1).cpu().numpy()  # (B, n_int - 1)
        assert not changed[1:].any(), "another tree's scores moved"
        np.testing.assert_array_equal(changed[0], reads)
        tested += 1
    assert tested >= 3
    # and the outside rows are read as given: O_u of move e
    out2 = out.clone()
    u = int(tab[0, 0, 0]) - nl
    out2[0, u] += 1.0
    got = eng.nni_scores(lvd, cd, 0.0, dp=f.dp, outside=out2)
    changed = (got != nni).any(dim=-1).cpu().numpy()
    np.testing.assert_array_equal(changed[0], tab[0, :, 0] == u + nl)
    assert not changed[1:].any()


def test_refusals(device):
    ch = random_topologies(2, 4, seed=0)
    L = 8
    eng = SankoffEngine(TreePlan(ch), L, 21, device)
    lv = torch.from_numpy(random_leaves(2, 4, L, 21, seed=1)).to(device)
    c = torch.from_numpy(int_cost(21, seed=2)).to(device)
    with pytest.raises(TrexError) as e:
        eng.nni_scores(lv, c, 0.0)
    assert e.value.code == TREX_E_UNSUPPORTED
    f = eng.forward(lv, c, 0.0)
    with pytest.raises(TrexError) as e:
        eng.outside(lv, c, 0.0, f.dp)
    assert e.value.code == TREX_E_UNSUPPORTED

    eng = SankoffEngine(TreePlan(ch), L, 4, device)
    lv = torch.from_numpy(random_leaves(2, 4, L, 4, seed=1)).to(device)
    c = torch.from_numpy(int_cost(4, seed=2)).to(device)
    f = eng.forward(lv, c, 0.0)
    out = eng.outside(lv, c, 0.0, f.dp)
    with pytest.raises(ValueError):
        eng.nni_scores(lv[:, :, :4].contiguous(), c, 0.0)
    with pytest.raises(ValueError):
        eng.nni_scores(lv, c[:3, :3].contiguous(), 0.0)
    with pytest.raises(ValueError):
        eng.nni_scores(lv, c, 0.0, dp=f.dp[:, :2].contiguous())
    with pytest.raises(ValueError):
        eng.nni_scores(lv, c, 0.0, dp=f.dp, outside=out.transpose(2, 3).contiguous())
    with pytest.raises(ValueError):
        eng.nni_scores(lv, c, 0.0, outside=out)
    with pytest.raises(ValueError):
        eng.outside(lv, c, 0.0, f.dp.double())
    with pytest.raises(TrexError):
        eng.nni_scores(lv, c, -1.0, dp=f.dp, outside=out)


@pytest.mark.parametrize("Q,tau", [(4, 0.0), (4, 0.5), (20, 0.0)])
def test_hill_climb(device, Q, tau):
    min_gain = 1e-5
    lv = simulate_leaves(8, 120, Q, 6, seed=11)[0][:8]
    ch = random_topologies(4, 8, seed=7)
    cost = hamming(4) if Q == 4 else int_cost(20, 3)
    res = nni_hill_climb(ch, lv, cost, tau=tau, device=device)
    assert res.children.shape == ch.shape
    assert res.rounds == res.n_moves.max() <= 9, (res.rounds, res.n_moves)
    cd = torch.from_numpy(cost).to(device)
    lvd = torch.from_numpy(lv).to(device)[None].expand(4, -1, -1).contiguous()
    ts = SankoffEngine(TreePlan(res.children), 120, Q, device).forward(lvd, cd, tau).tree_score
    assert np.array_equal(res.scores, ts.cpu().numpy())
    for b in range(4):
        h = res.history[b]
        assert all(y < x for x, y in zip(h, h[1:])), h
        assert len(h) == res.n_moves[b] + 1 and h[-1] == res.scores[b]
    assert res.n_moves.sum() >= 1
    if Q == 20:
        assert (res.n_moves >= 1).all()
    # a local optimum: no neighbour, scored by the engine's forward, gains more than min_gain
    moves = [(v, k) for v in range(8, 14) for k in (0, 1)]
    nb = np.stack([apply_nni(res.children[b], v, k) for b in range(4) for v, k in moves])
    nb_lv = lvd[:1].expand(len(nb), -1, -1).contiguous()
    nts = SankoffEngine(TreePlan(nb), 120, Q, device).forward(nb_lv, cd, tau).tree_score
    nts = nts.cpu().numpy().reshape(4, -1).astype(np.float64)
    s = res.scores.astype(np.float64)[:, None]
    assert (nts >= s - min_gain * np.abs(s)).all()
    if tau == 0.0:  # integer scores: the fp64 greedy takes the same path
        for b in range(4):
            ref_ch, ref_h = R.greedy_ref(ch[b], lv, cost, 0.0, min_gain)
            assert res.history[b] == ref_h, (b, res.history[b], ref_h)
            assert np.array_equal(res.children[b], ref_ch)
