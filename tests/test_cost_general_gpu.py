"""GPU parity of the Sankoff kernels on general cost matrices: asymmetric,
non-zero diagonal, min(C) != 0, fractional, negative (tests/_cases.py
general_cost) -- every other parity file builds C with hamming / int_cost
(symmetric, zero diagonal, min 0, small integers), on which C[child][parent]
for C[parent][child], a transposed dC, a K / K^T swap or a dropped min(C) are
invisible, and the branches the kernels take for a non-symmetric matrix never
run (sankoff.hip's general factored body behind cost_symmetric, the column
registers of sankoff_wide.hip's K mode, the K^T reads of the site kernels).

Each case first passes assert_cost_is_general on the CPU (the fp64 oracle
tells C from C^T on the case's own trees and leaves), then meets the suite's
bars against that oracle (tests/test_sankoff_gpu.py): hard DP table, site /
tree scores and trex-exact states bit-exact, hard dC rtol 1e-6, softmin scores
rtol 1e-5, DP table by assert_dp_close, dC by cond_rtol, marginals and soft
states by the conditioning bound.  Every check prints its worst err / bound.

Shapes: B = 3 topologies (tree 1 a caterpillar: the deepest stack), 6..16
taxa, L in {1, 70, 129, 257} (a partial second wave, a tile with few live
lanes), 4 % missing codes in some case of every kernel.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from _cases import (assert_cost_is_general, assert_dp_close, assert_grad_close,
                    assert_marginals_close, clear_argmax_mask, cond_rtol, general_cost,
                    random_leaves, random_topologies)
from oracle.sankoff_ref import backtrack_ref, run_dp_ref, run_sankoff_ref
from trex_amd import SankoffEngine, TreePlan, run_dp, run_sankoff, vectorized_dp, vmapped_backtrack
from trex_amd._lib import lib
from trex_amd.ragged import RaggedSankoffEngine, RaggedTreePlan
from trex_amd.topology import adjacency_from_children

pytestmark = pytest.mark.gpu

# tau of each softmin mode (tests/test_pair_tables_gpu.py MODES)
TAU = {"hard": 0.0, "factored": 0.5, "direct": 0.05, "general": 4000.0}


def caterpillar(n):
    ch = np.full((2 * n - 1, 2), -1, dtype=np.int32)
    ch[n] = (0, 1)
    for k in range(1, n - 1):
        ch[n + k] = (k + 1, n + k - 1)
    return ch


def _dev(x, device, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(device).contiguous()


@functools.lru_cache(maxsize=None)
def case(Q, mode, kind, n, L, missing, seed, hi=None):
    """Inputs and the fp64 reference of one case, built and guarded once and
    shared by the kernels that run it (read-only)."""
    tau = TAU[mode]
    B = 3
    ch = random_topologies(B, n, seed=100 * seed + n)
    ch[1] = caterpillar(n)
    leaves = random_leaves(B, n, L, Q, seed=100 * seed + L + Q, missing=missing)
    cost = general_cost(Q, seed, kind, hi=hi)
    if mode == "direct":
        assert (cost.max() - cost.min()) / tau > 40.0
    elif mode == "factored":
        assert (cost.max() - cost.min()) / tau < 40.0
    dts = np.linspace(0.5, 2.0, B)
    ref = assert_cost_is_general(cost, ch, leaves, tau, d_tree_score=dts,
                                 score_condition=mode != "general")
    return ch, leaves, cost, dts, ref


def _report(what, err, bound):
    print(f"  {what}: max err / bound {err:.3e} / {bound:.3e}")


def _exact(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    bad = int((got != want).sum())
    _report(what, float(bad), 0.0)
    np.testing.assert_array_equal(got, want, err_msg=what)


def _rel(got, want, rtol, what):
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    nz = want != 0  # an exact zero of the oracle has to come out as zero
    rel = np.abs(got - want)[nz] / np.abs(want)[nz]
    worst = float(rel.max()) if rel.size else 0.0
    _report(what, worst, rtol)
    bad = int((~(np.abs(got - want) <= rtol * np.abs(want))).sum())  # a NaN counts as bad
    assert bad == 0, f"{what}: {bad} entries above rtol {rtol:g}, worst {worst:.3e}"


def _trex_states(ch, leaves, cost):
    """run_sankoff_ref's ancestral states (B, n_int, L); a missing code is an
    out-of-range state (trex's all-1e5 row, not the wrap of a negative one)."""
    B, n, _ = leaves.shape
    Q = cost.shape[0]
    adj = adjacency_from_children(ch)
    seqs = np.where(leaves < 0, Q + 3, leaves).astype(np.float32)
    return np.stack([run_sankoff_ref(adj[b], cost, seqs[b], 2 * n - 1, Q, n,
                                     return_path=True)[0][n:] for b in range(B)])


def check_engine(device, ch, leaves, cost, dts_np, ref, tau):
    """forward, backward and the fused launch on one engine: fused == forward
    + backward bitwise, and every output against the fp64 oracle."""
    B, n, L = leaves.shape
    Q = cost.shape[0]
    eng = SankoffEngine(TreePlan(ch), L, Q, device)
    lv, c = _dev(leaves, device), _dev(cost, device, torch.float32)
    dts = _dev(dts_np, device, torch.float32)
    f = eng.forward(lv, c, tau, site_score=True)
    dc, mg, an = eng.backward(lv, c, tau, f.dp, dts, marginals=True, anc_states=True)
    f3, dc3, mg3, an3 = eng.fwd_bwd(lv, c, tau, dts, site_score=True, marginals=True,
                                    anc_states=True)
    torch.cuda.synchronize()
    for a, b, what in ((f3.dp, f.dp, "dp"), (f3.tree_score, f.tree_score, "tree"),
                       (f3.site_score, f.site_score, "site"), (dc3, dc, "dC"), (mg3, mg, "marg"),
                       (an3, an, "anc")):
        assert torch.equal(a, b), f"fused != forward + backward: {what}"
    got_dp = eng.state_rows(f.dp).cpu().numpy()
    got_mg = eng.state_rows(mg).cpu().numpy()
    if tau == 0.0:
        _exact(got_dp, ref["dp"].astype(np.float32), "hard dp")
        _exact(f.site_score.cpu().numpy(), ref["site_score"].astype(np.float32), "hard site score")
        _exact(f.tree_score.cpu().numpy(), ref["tree_score"].astype(np.float32), "hard tree score")
        _rel(dc.cpu().numpy(), ref["d_cost"], 1e-6, "hard dC")
        err = np.abs(got_mg - ref["marginals"]) / (1e-6 * np.abs(ref["marginals"]) + 1e-7)
        _report("hard marginals", float(err.max()), 1.0)
        assert err.max() <= 1.0
        anc = eng.backtrack(c, f.dp).cpu().numpy()
        _exact(anc.astype(np.float32), _trex_states(ch, leaves, cost), "trex states")
    else:
        _rel(f.tree_score.cpu().numpy(), ref["tree_score"], 1e-5, "tree score")
        _rel(f.site_score.cpu().numpy(), ref["site_score"], 1e-5, "site score")
        _report("dp", assert_dp_close(got_dp, ref), 1.0)
        rt = cond_rtol(ref["dp"], tau)
        _report("dC", assert_grad_close(dc.cpu().numpy(), ref["d_cost"], rtol=rt), rt)
        m = ref["marginals"]
        rel, mrt = assert_marginals_close(got_mg, m, ch, ref["dp"], tau)
        _report("marginals", rel, float(mrt.max()))
        clear = clear_argmax_mask(m, mrt)
        _exact(an.cpu().numpy()[clear], m.argmax(axis=2)[clear],
               f"soft states ({int(clear.sum())} of {clear.size} clear)")
    return f, dc


# ---------------------------------------------------------------------------
# Q <= 4: the lane-per-site kernel, the state-parallel quad (G = 4), staged
# ---------------------------------------------------------------------------
# (Q, mode, kind, n, L, missing, seed)
SMALL_CASES = [
    (2, "hard", "asym_int", 6, 257, 0.04, 1),
    (3, "hard", "asym_dyadic", 9, 129, 0.0, 1),
    (4, "hard", "neg", 16, 70, 0.04, 1),
    (4, "hard", "asym_int", 7, 1, 0.0, 1),
    (2, "factored", "asym_frac", 6, 257, 0.0, 1),
    (3, "factored", "neg", 9, 129, 0.0, 1),
    (4, "factored", "asym_dyadic", 16, 70, 0.0, 1),
    (4, "factored", "asym_frac", 7, 1, 0.0, 1),
    (3, "factored", "asym_int", 6, 70, 0.04, 1),
    (2, "direct", "asym_wide", 9, 70, 0.0, 1),
    (3, "direct", "asym_wide", 16, 129, 0.0, 1),
    (4, "direct", "asym_wide", 6, 257, 0.0, 1),
    (2, "general", "asym_int", 16, 70, 0.04, 1),
    (3, "general", "asym_frac", 6, 257, 0.0, 1),
    (4, "general", "asym_dyadic", 9, 129, 0.04, 1),
]


def _small_kernel(monkeypatch, kernel):
    if kernel == "lane-per-site":
        monkeypatch.setenv("TREX_WIDE_SMALLQ", "0")
    else:
        monkeypatch.setenv("TREX_WIDE_SMALLQ", "1")
        monkeypatch.setenv("TREX_STAGED", "1" if kernel == "staged" else "0")


def _id(c):
    return "-".join(str(x) for x in c[:5])


@pytest.mark.parametrize("kernel", ["lane-per-site", "state-parallel", "staged"])
@pytest.mark.parametrize("spec", SMALL_CASES, ids=_id)
def test_small_q_kernels(device, monkeypatch, spec, kernel):
    """Q = 2, 3, 4 on the three kernels the policy chooses between, in the
    hard, factored (the general sankoff_body<Q, kSoftK, 2 | 3, false, SYM =
    false> on the lane-per-site kernel), direct and general-leaf-table modes."""
    _small_kernel(monkeypatch, kernel)
    ch, leaves, cost, dts, ref = case(*spec)
    check_engine(device, ch, leaves, cost, dts, ref, TAU[spec[1]])


@pytest.mark.parametrize("Q,mode,kind,seed", [(2, "hard", "asym_dyadic", 1),
                                              (3, "factored", "asym_frac", 1),
                                              (4, "factored", "neg", 1),
                                              (4, "hard", "asym_int", 1),
                                              (2, "factored", "asym_int", 2),
                                              (3, "direct", "asym_wide", 1)])
def test_ragged_lane_per_site(device, Q, mode, kind, seed):
    """Two tree sizes in one ragged launch (the RAGGED = true bodies): per
    tree the DP table, scores, marginals and states against the oracle, dC
    against the trees' sum, fused == forward + backward bitwise."""
    tau = TAU[mode]
    sizes = [(7, 129), (12, 70)]
    chs = [random_topologies(1, n, seed=10 * seed + n)[0] for n, _ in sizes]
    chs[1] = caterpillar(12)
    leaves = [random_leaves(1, n, L, Q, seed=seed + L, missing=0.04 if tau == 0.0 else 0.0)[0]
              for n, L in sizes]
    cost = general_cost(Q, seed, kind)
    if mode == "direct":
        assert (cost.max() - cost.min()) / tau > 40.0
    dts = np.array([0.75, 1.5])
    refs = [assert_cost_is_general(cost, chs[b][None], leaves[b][None], tau, d_tree_score=dts[b:b + 1])
            for b in range(2)]
    plan = RaggedTreePlan(chs, [L for _, L in sizes])
    eng = RaggedSankoffEngine(plan, Q, device)
    lv = _dev(plan.pack_leaves(leaves), device)
    c = _dev(cost, device, torch.float32)
    d = _dev(dts, device, torch.float32)
    ts, dp, ss = eng.forward(lv, c, tau, site_score=True)
    dc, mg, an = eng.backward(lv, c, tau, dp, d, marginals=True, anc_states=True)
    ts3, dp3, ss3, dc3, mg3, an3 = eng.fwd_bwd(lv, c, tau, d, site_score=True, marginals=True,
                                               anc_states=True)
    torch.cuda.synchronize()
    for a, b, what in ((ts3, ts, "tree"), (dp3, dp, "dp"), (ss3, ss, "site"), (dc3, dc, "dC"),
                       (mg3, mg, "marg"), (an3, an, "anc")):
        assert torch.equal(a, b), f"fused != forward + backward: {what}"
    dpn, ssn, mgn, ann = (t.cpu().numpy() for t in (dp, ss, mg, an))
    ref_dc = sum(r["d_cost"] for r in refs)
    bt = eng.backtrack(c, dp).cpu().numpy() if tau == 0.0 else None
    rt = max(cond_rtol(r["dp"], tau) for r in refs) if tau > 0.0 else 1e-6
    for b, r in enumerate(refs):
        got_dp = plan.tree_rows(dpn, b).transpose(0, 2, 1)[None]
        got_mg = plan.tree_rows(mgn, b).transpose(0, 2, 1)[None]
        if tau == 0.0:
            _exact(got_dp, r["dp"].astype(np.float32), f"hard dp[{b}]")
            _exact(plan.tree_sites(ssn, b), r["site_score"][0].astype(np.float32), f"site[{b}]")
            _exact(ts[b].item(), np.float32(r["tree_score"][0]), f"tree[{b}]")
            _exact(plan.tree_rows(bt, b).astype(np.float32),
                   _trex_states(chs[b][None], leaves[b][None], cost)[0], f"trex states[{b}]")
        else:
            _rel(ts[b].item(), r["tree_score"][0], 1e-5, f"tree score[{b}]")
            _rel(plan.tree_sites(ssn, b), r["site_score"][0], 1e-5, f"site score[{b}]")
            _report(f"dp[{b}]", assert_dp_close(got_dp, r), 1.0)
            m = r["marginals"]
            rel, mrt = assert_marginals_close(got_mg, m, chs[b][None], r["dp"], tau)
            _report(f"marginals[{b}]", rel, float(mrt.max()))
            clear = clear_argmax_mask(m, mrt)
            _exact(plan.tree_rows(ann, b)[None][clear], m.argmax(axis=2)[clear], f"soft states[{b}]")
    if tau == 0.0:
        _rel(dc.cpu().numpy(), ref_dc, rt, "hard dC")
    else:
        _report("dC", assert_grad_close(dc.cpu().numpy(), ref_dc, rtol=rt), rt)


# ---------------------------------------------------------------------------
# Q > 4: the state-parallel kernel (G = 8 .. 64), staged, the site kernels
# ---------------------------------------------------------------------------
WIDE_CASES = [
    (5, "hard", "asym_int", 12, 129, 0.04, 1),
    (5, "factored", "asym_frac", 6, 257, 0.0, 1),
    (5, "direct", "asym_wide", 9, 70, 0.0, 1),
    (13, "hard", "asym_dyadic", 9, 70, 0.04, 1),
    (13, "factored", "neg", 12, 129, 0.0, 1),
    (13, "direct", "asym_wide", 6, 257, 0.0, 1),
    (20, "hard", "neg", 6, 257, 0.04, 2),
    (20, "factored", "asym_dyadic", 16, 70, 0.0, 1),
    (20, "direct", "asym_wide", 12, 129, 0.0, 1),
    (21, "hard", "asym_int", 16, 70, 0.0, 1),
    (21, "factored", "asym_frac", 9, 129, 0.04, 2),
    (21, "direct", "asym_wide", 7, 1, 0.0, 1),
    (61, "hard", "asym_dyadic", 7, 129, 0.04, 3),
    (61, "factored", "asym_int", 6, 70, 0.0, 2),
    (61, "direct", "asym_wide", 9, 257, 0.0, 1),
]


@pytest.mark.parametrize("kernel", ["wave", "staged"])
@pytest.mark.parametrize("spec", WIDE_CASES, ids=_id)
def test_wide_kernels(device, monkeypatch, spec, kernel):
    """G = 8, 16, 32, 64 on the one-wave-per-item and the staged kernel
    (TREX_SITE=0 keeps Q <= 20 off the site kernel): the factored cases run
    the K-mode wide_body with the column registers (fill_col_table, cf.cl,
    kdot_col<G, false>), which a symmetric matrix never takes."""
    monkeypatch.setenv("TREX_SITE", "0")
    monkeypatch.setenv("TREX_STAGED", "1" if kernel == "staged" else "0")
    ch, leaves, cost, dts, ref = case(*spec)
    check_engine(device, ch, leaves, cost, dts, ref, TAU[spec[1]])


BIGQ_CASES = [
    (65, "hard", "asym_int", 7, 70, 0.04, 1),
    (65, "factored", "asym_frac", 6, 129, 0.0, 2),
    (100, "direct", "asym_wide", 6, 70, 0.0, 1),
]


@pytest.mark.parametrize("spec", BIGQ_CASES, ids=_id)
def test_large_alphabet_kernel(device, spec):
    """64 < Q <= 128 (sankoff_bigq.hip): the same checks."""
    ch, leaves, cost, dts, ref = case(*spec)
    check_engine(device, ch, leaves, cost, dts, ref, TAU[spec[1]])


SITE_CASES = [
    (13, "factored", "asym_frac", 12, 257, 0.0, 2),
    (20, "factored", "asym_int", 16, 129, 0.04, 2),
    (20, "factored", "neg", 9, 70, 0.0, 2),
]


@pytest.mark.parametrize("site", ["1", "0"])
@pytest.mark.parametrize("spec", SITE_CASES, ids=_id)
def test_site_kernel_and_its_state_parallel_twin(device, monkeypatch, spec, site):
    """Q = 13 and 20, factored softmin: the MFMA lane-per-site kernel
    (TREX_SITE=1; its adjoint reads K^T as site_gate_write stored it) and the
    state-parallel kernel on the same inputs (TREX_SITE=0)."""
    monkeypatch.setenv("TREX_SITE", site)
    monkeypatch.setenv("TREX_STAGED", "0")
    monkeypatch.delenv("TREX_SITE2", raising=False)
    ch, leaves, cost, dts, ref = case(*spec)
    check_engine(device, ch, leaves, cost, dts, ref, TAU[spec[1]])


def _all_outputs(eng, lv, c, tau, dts):
    f, dc, mg, an = eng.fwd_bwd(lv, c, tau, dts, site_score=True, marginals=True, anc_states=True)
    f2 = eng.forward(lv, c, tau)
    dc2, _, _ = eng.backward(lv, c, tau, f2.dp, dts)
    torch.cuda.synchronize()
    return dict(dp=f.dp.clone(), tree=f.tree_score.clone(), site=f.site_score.clone(),
                dc=dc.clone(), marg=mg.clone(), anc=an.clone(), dp2=f2.dp.clone(), dc2=dc2.clone())


@pytest.mark.parametrize("knob", ["TREX_SITE_CHERRY", "TREX_SITE_SROW"])
def test_site_kernel_shortcuts_are_bitwise_neutral_asymmetric(device, monkeypatch, knob):
    """tests/test_sankoff_wide_gpu.py's comparison at Q = 20 on an asymmetric
    matrix: the cherry tables (a cherry of two equal codes i under state i
    costs 2 C[i][i] != 0) and the kept s rows are bitwise what they replace."""
    monkeypatch.setenv("TREX_SITE", "1")
    monkeypatch.delenv("TREX_SITE2", raising=False)
    ch, leaves, cost, dts_np, ref = case(*SITE_CASES[1])
    tau = 0.5
    L, Q = leaves.shape[2], cost.shape[0]
    lv, c = _dev(leaves, device), _dev(cost, device, torch.float32)
    dts = _dev(dts_np, device, torch.float32)
    runs = []
    for flag in ("1", "0"):
        monkeypatch.setenv(knob, flag)
        runs.append(_all_outputs(SankoffEngine(TreePlan(ch), L, Q, device), lv, c, tau, dts))
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    rt = cond_rtol(ref["dp"], tau)
    _report("dC", assert_grad_close(runs[0]["dc"].cpu().numpy(), ref["d_cost"], rtol=rt), rt)
    _report("dp", assert_dp_close(runs[0]["dp"].cpu().numpy().transpose(0, 1, 3, 2), ref), 1.0)


@pytest.mark.parametrize("spec", SITE_CASES[:2], ids=_id)
def test_site2_kernel_asymmetric(device, monkeypatch, spec):
    """The wave-pair kernel (TREX_SITE2=1; its launch counter shows that it
    took the calls) on asymmetric matrices: bitwise the one-wave kernel on
    everything but dC, every output against the oracle."""
    monkeypatch.setenv("TREX_SITE", "1")
    monkeypatch.setenv("TREX_STAGED", "0")
    ch, leaves, cost, dts_np, ref = case(*spec)
    tau = TAU[spec[1]]
    L, Q = leaves.shape[2], cost.shape[0]
    lv, c = _dev(leaves, device), _dev(cost, device, torch.float32)
    dts = _dev(dts_np, device, torch.float32)
    monkeypatch.setenv("TREX_SITE2", "0")
    n0 = lib().trex_debug_site2_launches()
    one = _all_outputs(SankoffEngine(TreePlan(ch), L, Q, device), lv, c, tau, dts)
    assert lib().trex_debug_site2_launches() == n0
    monkeypatch.setenv("TREX_SITE2", "1")
    check_engine(device, ch, leaves, cost, dts_np, ref, tau)
    assert lib().trex_debug_site2_launches() - n0 > 0
    pair = _all_outputs(SankoffEngine(TreePlan(ch), L, Q, device), lv, c, tau, dts)
    for k in ("dp", "tree", "site", "marg", "anc", "dp2"):
        assert torch.equal(pair[k], one[k]), k


# ---------------------------------------------------------------------------
# trex-exact backtrack: argmin_j (C[i][j] + D[j]), first index on ties
# ---------------------------------------------------------------------------
def _single_tree(Q, n, L, seed, hi):
    ch = random_topologies(1, n, seed=seed + Q)
    leaves = random_leaves(1, n, L, Q, seed=seed + L)
    cost = general_cost(Q, seed, "asym_int", hi=hi)
    assert_cost_is_general(cost, ch, leaves, 0.0)
    return ch[0], adjacency_from_children(ch)[0], leaves[0].astype(np.float32), cost


def _check_run_sankoff(device, Q, n, L, seed, hi):
    ch, adj, seqs, cost = _single_tree(Q, n, L, seed, hi)
    n_all = 2 * n - 1
    recon, dp, total = run_sankoff(adj, cost, seqs, n_all, Q, n, return_path=True, device=device)
    r_recon, r_dp, r_total = run_sankoff_ref(adj, cost, seqs, n_all, Q, n, return_path=True)
    _exact(dp.cpu().numpy(), r_dp, "dp")
    _exact(recon.cpu().numpy(), r_recon, "reconstruction")
    _exact(float(total), float(r_total), "total")
    return r_recon


@pytest.mark.parametrize("Q,n,L,seed,hi", [(2, 16, 257, 5, 2), (3, 9, 129, 1, 5), (4, 12, 70, 1, 5)])
def test_run_sankoff_split_lane_backtrack(device, Q, n, L, seed, hi):
    """run_sankoff(return_path=True) at Q <= 4: the split-lane backtrack
    kernel; Q = 2 with off-diagonal costs 1..2 (frequent first-index ties)."""
    _check_run_sankoff(device, Q, n, L, seed, hi)


@pytest.mark.parametrize("bt", ["split", "0"])
@pytest.mark.parametrize("Q,seed,hi", [(7, 1, 5), (20, 30, 2), (32, 2, 5)])
def test_backtrack_wide_asymmetric(device, monkeypatch, Q, seed, hi, bt):
    """The 8-lanes-per-site kernel and the one-lane-per-site one (TREX_BT4=0)."""
    if bt == "0":
        monkeypatch.setenv("TREX_BT4", "0")
    else:
        monkeypatch.delenv("TREX_BT4", raising=False)
    B, n, L = 3, 12, 129
    ch = random_topologies(B, n, seed=seed + Q)
    ch[1] = caterpillar(n)
    leaves = random_leaves(B, n, L, Q, seed=seed + L)
    cost = general_cost(Q, seed, "asym_int", hi=hi)
    ref = assert_cost_is_general(cost, ch, leaves, 0.0)
    eng = SankoffEngine(TreePlan(ch), L, Q, device)
    c = _dev(cost, device, torch.float32)
    f = eng.forward(_dev(leaves, device), c, 0.0)
    _exact(f.tree_score.cpu().numpy(), ref["tree_score"].astype(np.float32), "tree score")
    anc = eng.backtrack(c, f.dp).cpu().numpy()
    _exact(anc.astype(np.float32), _trex_states(ch, leaves, cost), "trex states")


@pytest.mark.parametrize("Q,seed,hi", [(4, 1, 2), (20, 1, 5), (61, 3, 5)])
def test_ragged_backtrack_asymmetric(device, Q, seed, hi):
    sizes = [(7, 129), (12, 70)]
    chs = [random_topologies(1, n, seed=seed + n)[0] for n, _ in sizes]
    leaves = [random_leaves(1, n, L, Q, seed=seed + L)[0] for n, L in sizes]
    cost = general_cost(Q, seed, "asym_int", hi=hi)
    refs = [assert_cost_is_general(cost, chs[b][None], leaves[b][None], 0.0) for b in range(2)]
    plan = RaggedTreePlan(chs, [L for _, L in sizes])
    eng = RaggedSankoffEngine(plan, Q, device)
    c = _dev(cost, device, torch.float32)
    ts, dp, _ = eng.forward(_dev(plan.pack_leaves(leaves), device), c, 0.0)
    _exact(ts.cpu().numpy(), np.array([r["tree_score"][0] for r in refs], np.float32), "tree score")
    an = eng.backtrack(c, dp).cpu().numpy()
    for b in range(2):
        _exact(plan.tree_rows(an, b).astype(np.float32),
               _trex_states(chs[b][None], leaves[b][None], cost)[0], f"trex states[{b}]")


def test_run_sankoff_past_the_engine_alphabet_asymmetric(device):
    """Q = 129: run_sankoff on the raw-table kernels (trex_run_dp,
    trex_backtrack_generic, trex_dp_root_total)."""
    _check_run_sankoff(device, 129, 12, 40, 3, 5)


@pytest.mark.parametrize("Q,seed,hi", [(4, 1, 2), (20, 1, 5), (33, 1, 5)])
def test_raw_tables_asymmetric(device, Q, seed, hi):
    """run_dp / vectorized_dp on the reference's own (L, n_all, Q) tables and
    the backtrack from them (Q = 33: the any-Q kernel)."""
    n, L = 9, 70
    ch, adj, seqs, cost = _single_tree(Q, n, L, seed, hi)
    n_all = 2 * n - 1
    dp0 = np.full((L, n_all, Q), 1e5, np.float32)
    bt0 = np.zeros((L, n_all, Q, 4), np.float32)
    r_dp, r_bt = run_dp_ref(adj, dp0, bt0, seqs, cost)
    dp, bt = vectorized_dp(adj, dp0, bt0, seqs, cost, device=device)
    _exact(dp.cpu().numpy(), r_dp, "dp")
    _exact(bt.cpu().numpy(), r_bt, "bt")
    dp1, bt1 = run_dp(adj, dp0[3], bt0[3], seqs[:, 3:4], cost, device=device)
    _exact(dp1.cpu().numpy(), r_dp[3], "run_dp dp")
    _exact(bt1.cpu().numpy(), r_bt[3], "run_dp bt")
    roots = r_dp[:, -1, :].argmin(axis=1).astype(np.int32)
    out = vmapped_backtrack(n_all - 1, None, bt, n_all, n, dp=dp)
    _exact(out.cpu().numpy(), backtrack_ref(n_all - 1, roots, r_bt, n_all, n), "states")


# ---------------------------------------------------------------------------
# min(C) in the factored softmin: C + s shifts the score by s per edge
# ---------------------------------------------------------------------------
FAMILIES = {
    "lane-per-site": (4, {"TREX_WIDE_SMALLQ": "0"}),
    "state-parallel-G4": (3, {"TREX_WIDE_SMALLQ": "1", "TREX_STAGED": "0"}),
    "wide-G32": (21, {"TREX_SITE": "0", "TREX_STAGED": "0"}),
    "site": (20, {"TREX_SITE": "1", "TREX_STAGED": "0"}),
}


# the site kernel takes softmin calls only
SHIFT_CASES = [(fam, tau) for fam in FAMILIES for tau in (0.0, 0.5) if (fam, tau) != ("site", 0.0)]


@pytest.mark.parametrize("family,tau", SHIFT_CASES)
def test_shifted_cost_shifts_the_score(device, monkeypatch, family, tau):
    """No oracle: for C' = C + s the score of a tree moves by s per edge per
    site, s (n_all - 1) L -- exactly in hard mode (dyadic C and s), to rtol
    1e-5 of |score'| under the softmin -- and dC stays (softmin weights are
    shift-invariant) to the softmin bar.  A dropped or sign-flipped min(C) in
    base = md + cmin / K = exp2((cmin - c) a) breaks both."""
    Q, env = FAMILIES[family]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("TREX_SITE2", raising=False)
    B, n, L = 3, 9, 129
    ch = random_topologies(B, n, seed=Q)
    ch[1] = caterpillar(n)
    leaves = random_leaves(B, n, L, Q, seed=Q + 1)
    cost = general_cost(Q, 3, "asym_dyadic")
    assert_cost_is_general(cost, ch, leaves, tau)
    eng = SankoffEngine(TreePlan(ch), L, Q, device)
    lv = _dev(leaves, device)
    f, dc, _, _ = eng.fwd_bwd(lv, _dev(cost, device, torch.float32), tau)
    ts, dcn = f.tree_score.cpu().numpy().astype(np.float64), dc.cpu().numpy()
    rt = cond_rtol(f.dp.cpu().numpy(), tau) if tau > 0.0 else 1e-6
    for s in (1.5, -0.75):
        shifted = (cost + np.float32(s)).astype(np.float32)
        assert shifted.min() != 0
        f2, dc2, _, _ = eng.fwd_bwd(lv, _dev(shifted, device, torch.float32), tau)
        ts2 = f2.tree_score.cpu().numpy().astype(np.float64)
        want = s * (2 * n - 2) * L
        if tau == 0.0:
            _exact(ts2 - ts, np.full(B, want), f"s = {s}: score shift")
        else:
            err = np.abs(ts2 - ts - want) / np.abs(ts2)
            _report(f"s = {s}: score shift", float(err.max()), 1e-5)
            assert (err <= 1e-5).all()
        _report(f"s = {s}: dC", assert_grad_close(dc2.cpu().numpy(), dcn, rtol=rt), rt)
