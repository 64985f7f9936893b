"""GPU tests of the attachment scores (sankoff_nni.hip, attach_score_kernel),
stepwise_addition and parsimony_search: against the fp64 references of
_attach_ref.py (hard mode with integer costs: exact), against the engine's own
forward on rebuilt topologies, whole subtrees through sub_rows, softmin,
reproducibility, refusals, the builders against an fp64 greedy."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import _attach_ref as A
import _nni_ref as R
from _cases import (assert_cost_is_general, cond_rtol, general_cost, hamming, int_cost,
                    random_leaves, random_topologies, simulate_leaves)
from test_nni_gpu import SHAPES, case as nni_case
from trex_amd import (SankoffEngine, TreePlan, TrexError, insert_leaf, nni_hill_climb,
                      parsimony_search, stepwise_addition)
from trex_amd._lib import TREX_E_UNSUPPORTED

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(n, L, Q, tau, missing=None):
    """test_nni_gpu's inputs (B = 3 topologies, missing codes at n = 6,
    asymmetric costs with a non-zero diagonal in every case), the new leaf =
    row n of random_leaves(3, n + 1), and the fp64 references; computed once
    per case, read-only."""
    ch, lv, cost, _ = nni_case(n, L, Q, tau, missing)
    hard = tau == 0.0
    if missing is None:
        missing = 0.05 if (hard and n == 6) else 0.0
    new = random_leaves(3, n + 1, L, Q, seed=n + L, missing=missing)
    new = np.ascontiguousarray(new[:, n])
    ref = np.stack([A.attach_ref(ch[b], lv[b], cost, tau, new_codes=new[b]) for b in range(3)])
    bf = np.stack([A.brute_force(ch[b], np.concatenate([lv[b], new[b][None]]), cost, tau)
                   for b in range(3)])
    return ch, lv, cost, new, ref, bf


def run(device, ch, lv, cost, new, tau):
    eng = SankoffEngine(TreePlan(ch), lv.shape[2], cost.shape[0], device)
    lvd = torch.from_numpy(lv).to(device)
    cd = torch.from_numpy(cost).to(device)
    nd = torch.from_numpy(new).to(device)
    f = eng.forward(lvd, cd, tau)
    out = eng.outside(lvd, cd, tau, f.dp)
    sc = eng.attach_scores(lvd, cd, tau, new_leaf=nd, dp=f.dp, outside=out)
    torch.cuda.synchronize()
    return eng, lvd, cd, nd, f, out, sc


@pytest.mark.parametrize("n,L,Q", SHAPES)
def test_hard_mode_is_exact(device, n, L, Q):
    ch, lv, cost, new, ref, bf = case(n, L, Q, 0.0)
    eng, lvd, cd, nd, f, out, sc = run(device, ch, lv, cost, new, 0.0)
    assert float(ref.max()) < 2 ** 24  # integers exact in fp32
    assert sc.shape == (3, 2 * n - 1) and sc.dtype == torch.float32
    assert torch.equal(sc.cpu(), torch.from_numpy(ref.astype(np.float32))), "attach_ref"
    assert torch.equal(sc.cpu(), torch.from_numpy(bf.astype(np.float32))), "brute force"
    # attach_scores runs the forward and the outside pass itself when not given
    assert torch.equal(eng.attach_scores(lvd, cd, 0.0, new_leaf=nd), sc)
    assert torch.equal(eng.attach_scores(lvd, cd, 0.0, new_leaf=nd, dp=f.dp), sc)


def test_hard_mode_equals_engine_forward_on_rebuilt_trees(device):
    B, n, L, Q = 16, 32, 300, 4
    ch = random_topologies(B, n, seed=31)
    lv = random_leaves(B, n + 1, L, Q, seed=32)
    cost = int_cost(Q, seed=33)
    lvd = torch.from_numpy(lv).to(device)
    cd = torch.from_numpy(cost).to(device)
    sc = SankoffEngine(TreePlan(ch), L, Q, device).attach_scores(
        lvd[:, :n].contiguous(), cd, 0.0, new_leaf=lvd[:, n].contiguous())
    assert sc.shape == (B, 2 * n - 1)
    grown = np.stack([insert_leaf(ch[b], x) for b in range(B) for x in range(2 * n - 1)])
    g_lv = lvd.repeat_interleave(2 * n - 1, dim=0).contiguous()
    ts = SankoffEngine(TreePlan(grown), L, Q, device).forward(g_lv, cd, 0.0).tree_score
    assert torch.equal(sc.reshape(-1), ts)
    assert len(torch.unique(sc)) > 10  # the edge does change the score


def test_one_hot_sub_rows_give_the_bits_of_new_leaf(device):
    for tau in (0.0, 0.5):
        ch, lv, cost, new, _, _ = case(6, 70, 4, tau)  # tau = 0: with missing codes
        eng, lvd, cd, nd, f, out, sc = run(device, ch, lv, cost, new, tau)
        rows = torch.from_numpy(A.leaf_rows(new.reshape(-1), 4).astype(np.float32))
        rows = rows.reshape(3, 70, 4).to(device)
        got = eng.attach_scores(lvd, cd, tau, sub_rows=rows, dp=f.dp, outside=out)
        assert torch.equal(got, sc)


SUBTREE_CASES = [(4, 0.0, 44), (5, 0.0, 1), (4, 0.5, 44), (5, 0.5, 44)]  # Q, tau, cost seed


def test_a_whole_subtree_through_sub_rows(device):
    """Tree S (3 leaves) attached on every edge of tree A (6 leaves): the
    regraft half of an SPR move.  Asymmetric costs; Q = 4 and Q = 5 (the
    padded kernel's sub_rows read); tau = 0 with integer costs: exact,
    tau = 0.5: within 1e-5 of the fp64 forward on the grafted trees."""
    L = 70
    cha = random_topologies(1, 6, seed=41)
    chs = random_topologies(1, 3, seed=42)
    for Q, tau, seed in SUBTREE_CASES:
        lv = random_leaves(1, 9, L, Q, seed=43)  # disjoint rows: A 0..5, S 6..8
        cost = general_cost(Q, seed, "asym_int" if tau == 0.0 else "asym_frac")
        assert_cost_is_general(cost, cha, lv[:, :6], tau)
        cd = torch.from_numpy(cost).to(device)
        lva = torch.from_numpy(lv[:, :6]).to(device).contiguous()
        lvs = torch.from_numpy(lv[:, 6:]).to(device).contiguous()
        rows = SankoffEngine(TreePlan(chs), L, Q, device).forward(lvs, cd, tau).dp[:, -1].contiguous()
        assert rows.shape == (1, L, Q)
        sc = SankoffEngine(TreePlan(cha), L, Q, device).attach_scores(lva, cd, tau, sub_rows=rows)
        want = np.array([R.sankoff_fwd_bwd_ref(A.graft_ref(cha[0], chs[0], x), lv[0], cost,
                                               tau)["tree_score"] for x in range(11)])
        assert len(np.unique(want)) > 3
        if tau == 0.0:
            assert want.max() < 2 ** 24
            assert torch.equal(sc.cpu()[0], torch.from_numpy(want.astype(np.float32))), (Q, tau)
        else:
            rel = np.abs(sc.cpu().numpy()[0].astype(np.float64) - want) / np.abs(want)
            print(f"subtree through sub_rows Q={Q} tau={tau}: worst rel err {rel.max():.3e}")
            assert rel.max() <= 1e-5, (Q, tau, rel.max())


@pytest.mark.parametrize("n,L,Q", SHAPES)  # Q = 2, 3; Q = 5: the padded soft kernel, dead states
def test_softmin_within_1e5_of_fp64_brute_force(device, n, L, Q):
    tau = 0.5
    ch, lv, cost, new, ref, bf = case(n, L, Q, tau)
    eng, lvd, cd, nd, f, out, sc = run(device, ch, lv, cost, new, tau)
    got = sc.cpu().numpy().astype(np.float64)
    rel = np.abs(got - bf) / np.abs(bf)
    print(f"attach softmin n={n} L={L} Q={Q}: worst rel err {rel.max():.3e}")
    assert rel.max() <= 1e-5, f"attachment scores: worst rel err {rel.max():.3e}"


def test_softmin_with_missing_codes(device):
    """5 % missing codes (the new leaf's too) under the softmin: the bar is
    max(1e-5, cond_rtol) -- fp32 D carries trex's 1e5 offsets -- and the fp64
    outside-table reference alone meets it against the fp64 brute force."""
    n, L, Q, tau = 6, 70, 4, 0.5
    ch, lv, cost, new, ref, bf = case(n, L, Q, tau, 0.05)
    assert (lv < 0).any() and (new < 0).any()
    dmax = max(float(np.abs(r["inside"]).max()) for r in nni_case(n, L, Q, tau, 0.05)[3])
    bar = max(1e-5, cond_rtol(np.array([dmax]), tau))
    rel_ref = np.abs(ref - bf) / np.abs(bf)
    assert rel_ref.max() <= bar, f"fp64 reference vs brute force: {rel_ref.max():.3e} > {bar:.3e}"
    eng, lvd, cd, nd, f, out, sc = run(device, ch, lv, cost, new, tau)
    rel = np.abs(sc.cpu().numpy().astype(np.float64) - bf) / np.abs(bf)
    print(f"attach softmin with missing codes: fp64 reference {rel_ref.max():.3e}, device "
          f"{rel.max():.3e}, bar {bar:.3e}")
    assert rel.max() <= bar, f"attachment scores: worst rel err {rel.max():.3e} > {bar:.3e}"


@pytest.mark.parametrize("tau", [0.0, 0.5])
def test_repeated_calls_are_bitwise_equal(device, tau):
    ch, lv, cost, new, _, _ = case(9, 129, 4, tau)
    eng, lvd, cd, nd, f, out, sc = run(device, ch, lv, cost, new, tau)
    for _ in range(2):
        assert torch.equal(eng.attach_scores(lvd, cd, tau, new_leaf=nd, dp=f.dp, outside=out), sc)
    assert torch.equal(eng.attach_scores(lvd, cd, tau, new_leaf=nd), sc)


def test_scores_are_computed_from_the_callers_table(device):
    ch, lv, cost, new, _, _ = case(9, 129, 4, 0.0)
    eng, lvd, cd, nd, f, out, sc = run(device, ch, lv, cost, new, 0.0)
    nl = eng.plan.n_leaves
    for b, r in ((0, 2), (1, 7), (2, 4)):  # (1, 7): the root's row
        out2 = out.clone()
        out2[b, r] += 1.0
        got = eng.attach_scores(lvd, cd, 0.0, new_leaf=nd, dp=f.dp, outside=out2)
        changed = (got != sc).cpu().numpy()  # (B, n_all)
        want = np.zeros_like(changed)
        want[b, ch[b, nl + r]] = True  # the two child edges of that node, in that tree only
        np.testing.assert_array_equal(changed, want)


def test_refusals(device):
    ch = random_topologies(2, 4, seed=0)
    L = 8
    eng = SankoffEngine(TreePlan(ch), L, 21, device)
    lv = torch.from_numpy(random_leaves(2, 4, L, 21, seed=1)).to(device)
    c = torch.from_numpy(int_cost(21, seed=2)).to(device)
    new = lv[:, 0].contiguous()
    with pytest.raises(TrexError) as e:
        eng.attach_scores(lv, c, 0.0, new_leaf=new)
    assert e.value.code == TREX_E_UNSUPPORTED
    f = eng.forward(lv, c, 0.0)
    with pytest.raises(TrexError) as e:
        eng.attach_scores(lv, c, 0.0, new_leaf=new, dp=f.dp, outside=torch.zeros_like(f.dp))
    assert e.value.code == TREX_E_UNSUPPORTED
    with pytest.raises(TrexError) as e:
        stepwise_addition(lv[0].cpu().numpy(), c.cpu().numpy(), device=device)
    assert e.value.code == TREX_E_UNSUPPORTED

    eng = SankoffEngine(TreePlan(ch), L, 4, device)
    lv = torch.from_numpy(random_leaves(2, 4, L, 4, seed=1)).to(device)
    c = torch.from_numpy(int_cost(4, seed=2)).to(device)
    new = lv[:, 0].contiguous()
    rows = torch.zeros((2, L, 4), dtype=torch.float32, device=device)
    f = eng.forward(lv, c, 0.0)
    out = eng.outside(lv, c, 0.0, f.dp)
    bad = [
        dict(),  # neither
        dict(new_leaf=new, sub_rows=rows),  # both
        dict(new_leaf=new[:, :4].contiguous()),
        dict(new_leaf=new.to(torch.int32)),
        dict(new_leaf=new.cpu()),
        dict(new_leaf=lv.transpose(0, 1)[0]),  # not contiguous
        dict(sub_rows=rows[:, :, :3].contiguous()),
        dict(sub_rows=rows.double()),
        dict(sub_rows=rows.transpose(1, 2)),
        dict(new_leaf=new, dp=f.dp[:, :2].contiguous()),
        dict(new_leaf=new, dp=f.dp, outside=out.transpose(2, 3).contiguous()),
        dict(new_leaf=new, outside=out),  # outside without dp
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            eng.attach_scores(lv, c, 0.0, **kw)
    with pytest.raises(ValueError):
        eng.attach_scores(lv[:, :, :4].contiguous(), c, 0.0, new_leaf=new)
    with pytest.raises(ValueError):
        eng.attach_scores(lv, c[:3, :3].contiguous(), 0.0, new_leaf=new)
    with pytest.raises(TrexError):
        eng.attach_scores(lv, c, -1.0, new_leaf=new, dp=f.dp, outside=out)


def _stepwise_data(Q):
    lv = simulate_leaves(8, 120, Q, 6, seed=11)[0][:8]
    cost = hamming(4) if Q == 4 else int_cost(20, 3)
    rng = np.random.default_rng(5)
    order = np.stack([np.arange(8), np.arange(8)[::-1], rng.permutation(8), rng.permutation(8)])
    return lv, cost, order


def _forward(device, ch, lv, cost, tau):
    lvd = torch.from_numpy(lv).to(device)[None].expand(len(ch), -1, -1).contiguous()
    eng = SankoffEngine(TreePlan(ch), lv.shape[1], cost.shape[0], device)
    return eng.forward(lvd, torch.from_numpy(cost).to(device), tau).tree_score.cpu().numpy()


@pytest.mark.parametrize("Q", [4, 20])
def test_stepwise_addition_hard(device, Q):
    lv, cost, order = _stepwise_data(Q)
    res = stepwise_addition(lv, cost, order=order, device=device)
    assert res.children.shape == (4, 15, 2) and res.children.dtype == np.int32
    assert res.scores.shape == (4,) and res.scores.dtype == np.float32
    assert np.array_equal(res.order, order)
    for b in range(4):
        ref_ch, ref_score = A.stepwise_ref(lv, cost, order[b], 0.0)
        assert np.array_equal(res.children[b], ref_ch), b
        assert res.scores[b] == ref_score, (b, res.scores[b], ref_score)
    assert np.array_equal(res.scores, _forward(device, res.children, lv, cost, 0.0))
    rand = _forward(device, random_topologies(4, 8, seed=7), lv, cost, 0.0)
    print(f"stepwise Q={Q}: {res.scores.tolist()} against random trees {rand.tolist()}")
    assert res.scores.max() < rand.min()
    # order=None: tree 0 takes the taxa as given, the others default_rng(seed) permutations
    auto = stepwise_addition(lv, cost, n_trees=3, seed=9, device=device)
    rng = np.random.default_rng(9)
    want = np.stack([np.arange(8), rng.permutation(8), rng.permutation(8)])
    assert np.array_equal(auto.order, want)
    assert np.array_equal(auto.children[0], res.children[0])


def test_stepwise_addition_ties_occur():
    """With hamming costs the fp64 attachment scores of the test data tie at
    the minimum, so the lowest-node-id rule decides (reference side only)."""
    lv, cost, order = _stepwise_data(4)
    taxa = lv[order[0]]
    start = [R.sankoff_fwd_bwd_ref(t, taxa[:3], cost, 0.0)["tree_score"] for t in A.TRIPLETS]
    ch = A.TRIPLETS[int(np.argmin(start))]
    ties = 0
    for k in range(3, 8):
        sc = A.attach_ref(ch, taxa[:k], cost, 0.0, new_codes=taxa[k])
        ties += int((sc == sc.min()).sum() > 1)
        ch = A.insert_leaf_ref(ch, int(np.argmin(sc)))
    assert ties >= 1


@pytest.mark.parametrize("Q", [4, 20])
def test_stepwise_addition_softmin(device, Q):
    lv, cost, order = _stepwise_data(Q)
    res = stepwise_addition(lv, cost, order=order, tau=0.5, device=device)
    assert res.children.shape == (4, 15, 2)
    for b in range(4):
        ch = res.children[b]
        for node in range(8, 15):
            assert 0 <= ch[node, 0] < ch[node, 1] < node
        assert sorted(ch[8:].reshape(-1)) == list(range(14))  # every taxon and node once
        assert max(R.leaf_sets(ch), key=len) == frozenset(range(8))
    TreePlan(res.children).nni_host  # proper trees
    assert np.array_equal(res.scores, _forward(device, res.children, lv, cost, 0.5))


@pytest.mark.parametrize("tau", [0.0, 0.5])
def test_parsimony_search(device, tau):
    lv, cost, _ = _stepwise_data(4)
    res = parsimony_search(lv, cost, n_trees=4, seed=3, tau=tau, device=device)
    start = stepwise_addition(lv, cost, n_trees=4, seed=3, tau=tau, device=device)
    climb = nni_hill_climb(start.children, lv, cost, tau=tau, device=device)
    assert np.array_equal(res.start_scores, start.scores)
    assert np.array_equal(res.order, start.order)
    assert np.array_equal(res.children, climb.children)
    assert np.array_equal(res.scores, climb.scores)
    assert res.history == climb.history and res.rounds == climb.rounds
    assert np.array_equal(res.n_moves, climb.n_moves)
    assert (res.scores <= res.start_scores).all()
