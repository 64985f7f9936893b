"""Guard-band tests: the Sankoff kernels stay inside their buffers.

Every case runs one call three times with the same environment
(tests/_guard.py): R0 on the engine method's own buffers, R1 and R2 through
the C ABI on buffers between 1 MiB canaries, with different guard and prefill
bytes.  R1 == R2 == R0 bitwise, every guard intact (inputs, outputs,
workspaces of exactly the ``*_workspace_bytes`` size), every input unchanged.
No oracle and no tolerance: the values are pinned by the parity files.

Shapes: L in {1, 67, 68} -- 67 is prime (a partial last tile of every
sites-per-wave the kernels use, L % 4 != 0: the per-lane leaf loader), 68 a
4-site last tile with L % 4 == 0 (the dword leaf prefetch over-reads the row
tail), 1 the degenerate tile; B = 3 topologies of 5 leaves, tree 1 a
caterpillar, 5 % missing codes; one 80-leaf case (> kPrefetchRows) at L = 68.
Costs: general_cost "asym_int" at tau = 0, "asym_frac" at tau = 0.5.

Entry point / family -> test ids:

    trex_sankoff_fwd, _bwd, _fwd_bwd,        test_uniform[<family>-<tau>-<n>x<L>]: the five
    trex_sankoff_backtrack,                  phases of one family, tau and shape
    trex_dp_to_trex_layout
      Q = 2, 3, 4 lane-per-site              q2-lane, q3-lane, q4-lane (TREX_DEFER default),
                                             q2-lane-defer0, q3-lane-defer0, q4-lane-defer0
      Q = 2, 3, 4 state-parallel G = 4       q2-sp, q3-sp, q4-sp
      Q = 2, 3, 4 staged                     q2-staged, q3-staged, q4-staged
      state-parallel G = 8 .. 64             q5-sp, q13-sp, q20-sp (4 idle lanes), q21-sp, q61-sp
      staged, Q > 4                          q20-staged
      site kernel (tau = 0.5)                q13-site, q20-site, and -cherry0, -srow0, -minws
                                             (the smallest accepted workspace) of each
      wave-pair site kernel                  q20-site2 (trex_debug_site2_launches moves)
      large alphabet                         q100-big
      backtrack twins                        q4-bt4off, q20-bt4off, q61-bt4off (TREX_BT4=0; the
                                             split-lane kernels run in every other family)
      80 leaves, L = 68                      the q4-lane, q4-lane-defer0, q4-sp, q4-staged ids
                                             with shape 80x68
    persistent forward, second item          test_persistent_forward_second_item_per_wave
    trex_sankoff_outside, _nni, _attach      test_outside_nni_attach[q<Q>-<tau>-<n>x<L>]
      (new_leaf and sub_rows)
    trex_sankoff_ragged (1 / 2 / 3),         test_ragged[q<Q>-<tau>]
    trex_sankoff_ragged_backtrack
    trex_run_dp, trex_backtrack_generic,     test_raw_tables[q4], [q130]
    trex_dp_root_total
    captured replay                          test_captured_replay[...]
    the harness on the device                test_harness_flags_*_on_the_device
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import _guard as G
from _cases import general_cost, random_leaves, random_topologies
from trex_amd import SankoffEngine, TreePlan, vectorized_dp, vmapped_backtrack
from trex_amd._lib import check, lib, ptr, stream_handle
from trex_amd.ragged import RaggedSankoffEngine, RaggedTreePlan
from trex_amd.topology import adjacency_from_children, children_from_adjacency

pytestmark = pytest.mark.gpu

KNOBS = ("TREX_WIDE_SMALLQ", "TREX_STAGED", "TREX_SITE", "TREX_SITE2", "TREX_SITE_CHERRY",
         "TREX_SITE_SROW", "TREX_DEFER", "TREX_BT4")


def _env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def caterpillar(n):
    ch = np.full((2 * n - 1, 2), -1, dtype=np.int32)
    ch[n] = (0, 1)
    for k in range(1, n - 1):
        ch[n + k] = (k + 1, n + k - 1)
    return ch


@functools.lru_cache(maxsize=None)
def inputs(Q, n, L, soft, B=3):
    """(children, leaves, cost, d_tree_score) of one case, host arrays."""
    ch = random_topologies(B, n, seed=7 * n + L)
    ch[1] = caterpillar(n)
    leaves = random_leaves(B, n, L, Q, seed=100 * Q + L + n, missing=0.05)
    cost = general_cost(Q, 1, "asym_frac" if soft else "asym_int")
    dts = np.linspace(0.5, 2.0, B).astype(np.float32)
    return ch, leaves, cost, dts


def _dev(x, device):
    return torch.as_tensor(np.ascontiguousarray(x)).to(device).contiguous()


# ---------------------------------------------------------------------------
# the harness itself, once on the device (torch indexing inside the allocation)
# ---------------------------------------------------------------------------
def _stand_in(run, x, *, short=0, past=False):
    xi = run.input("x", x)
    out = run.output("out", (x.size,), torch.float32)
    n = x.size - short
    out[:n].copy_(2.0 * xi[:n].to(torch.float32) + 1.0)
    if past:
        h = run.outputs["out"]
        h.flat[G.GUARD_BYTES + h.nbytes] = 0
    return out


def test_harness_flags_a_store_one_past_the_payload_on_the_device(device):
    x = (np.arange(67) % 4).astype(np.int8)
    r0 = lambda: {"out": _dev(2.0 * x.astype(np.float32) + 1.0, device)}  # noqa: E731
    G.protocol(device, r0, lambda run: _stand_in(run, x))
    with pytest.raises(AssertionError,
                       match=r"output out.*first at offset 268, last at offset 268 "):
        G.protocol(device, r0, lambda run: _stand_in(run, x, past=True))


def test_harness_flags_an_unwritten_last_entry_on_the_device(device):
    x = (np.arange(67) % 4).astype(np.int8)
    r0 = lambda: {"out": _dev(2.0 * x.astype(np.float32) + 1.0, device)}  # noqa: E731
    with pytest.raises(AssertionError, match=r"out: R1 vs R2.*1 of 67 entries differ, first at "
                                             r"flat index 66 "):
        G.protocol(device, r0, lambda run: _stand_in(run, x, short=1))


# ---------------------------------------------------------------------------
# uniform engine: fwd, bwd, fused, backtrack, layout adapter
# ---------------------------------------------------------------------------
_LANE = {"TREX_WIDE_SMALLQ": "0"}
_SP4 = {"TREX_WIDE_SMALLQ": "1", "TREX_STAGED": "0"}
_ST4 = {"TREX_WIDE_SMALLQ": "1", "TREX_STAGED": "1"}
_WIDE = {"TREX_SITE": "0", "TREX_STAGED": "0"}
_SITE = {"TREX_SITE": "1", "TREX_STAGED": "0"}

# name -> (Q, env, taus)
FAMILIES = {}
for _q in (2, 3, 4):
    FAMILIES[f"q{_q}-lane"] = (_q, _LANE, (0.0, 0.5))
    FAMILIES[f"q{_q}-lane-defer0"] = (_q, dict(_LANE, TREX_DEFER="0"), (0.0, 0.5))
    FAMILIES[f"q{_q}-sp"] = (_q, _SP4, (0.0, 0.5))
    FAMILIES[f"q{_q}-staged"] = (_q, _ST4, (0.0, 0.5))
for _q in (5, 13, 20, 21, 61):
    FAMILIES[f"q{_q}-sp"] = (_q, _WIDE, (0.0, 0.5))
FAMILIES["q20-staged"] = (20, {"TREX_SITE": "0", "TREX_STAGED": "1"}, (0.0, 0.5))
for _q in (13, 20):
    FAMILIES[f"q{_q}-site"] = (_q, _SITE, (0.5,))
    FAMILIES[f"q{_q}-site-cherry0"] = (_q, dict(_SITE, TREX_SITE_CHERRY="0"), (0.5,))
    FAMILIES[f"q{_q}-site-srow0"] = (_q, dict(_SITE, TREX_SITE_SROW="0"), (0.5,))
    FAMILIES[f"q{_q}-site-minws"] = (_q, _SITE, (0.5,))
FAMILIES["q20-site2"] = (20, dict(_SITE, TREX_SITE2="1"), (0.5,))
FAMILIES["q100-big"] = (100, {}, (0.0, 0.5))
FAMILIES["q4-bt4off"] = (4, dict(_LANE, TREX_BT4="0"), (0.0,))
FAMILIES["q20-bt4off"] = (20, dict(_WIDE, TREX_BT4="0"), (0.0,))
FAMILIES["q61-bt4off"] = (61, dict(_WIDE, TREX_BT4="0"), (0.0,))

SHAPES = [(5, 1), (5, 67), (5, 68)]
UNIFORM = [(fam, tau, n, L) for fam, (_, _, taus) in FAMILIES.items() for tau in taus
           for n, L in SHAPES]
# > kPrefetchRows leaves: the Q <= 4 kernels' leaf tile without the prefetch
UNIFORM += [(fam, tau, 80, 68) for fam in ("q4-lane", "q4-lane-defer0", "q4-sp", "q4-staged")
            for tau in (0.0, 0.5)]


def _uid(c):
    return f"{c[0]}-{c[1]}-{c[2]}x{c[3]}"


@pytest.mark.parametrize("fam,tau,n,L", UNIFORM, ids=[_uid(c) for c in UNIFORM])
def test_uniform(device, monkeypatch, fam, tau, n, L):
    Q, env, _ = FAMILIES[fam]
    _env(monkeypatch, env)
    ch, leaves, cost, dts = inputs(Q, n, L, tau > 0.0)
    plan = TreePlan(ch)  # under the environment: TREX_DEFER is read by the planner
    eng = SankoffEngine(plan, L, Q, device)
    lv, c, d = _dev(leaves, device), _dev(cost, device), _dev(dts, device)
    wsb = None
    if fam.endswith("minws"):
        # the smallest accepted workspace: no room for the kept s rows, the
        # guard directly behind the cherry tables
        wsb = (int(lib().trex_workspace_bytes(plan.B, L, plan.n_all, Q))
               - plan.B * plan.n_int * L * Q * 4)
    site2_before = lib().trex_debug_site2_launches()

    def r0_fwd():
        f = eng.forward(lv, c, tau, site_score=True)
        return dict(dp=f.dp, site_score=f.site_score, tree_score=f.tree_score)

    dp = G.protocol(device, r0_fwd, lambda run: G.sankoff_fwd(
        run, plan, leaves, cost, L, Q, tau, workspace_bytes=wsb))["dp"]
    dp_dev = dp.to(device)

    def r0_bwd():
        dc, mg, an = eng.backward(lv, c, tau, dp_dev, d, marginals=True, anc_states=True)
        return dict(d_cost=dc, marginals=mg, anc_states=an)

    G.protocol(device, r0_bwd, lambda run: G.sankoff_bwd(
        run, plan, leaves, cost, L, Q, tau, dp, dts, workspace_bytes=wsb))

    def r0_fused():
        f, dc, mg, an = eng.fwd_bwd(lv, c, tau, d, site_score=True, marginals=True,
                                    anc_states=True)
        return dict(dp=f.dp, site_score=f.site_score, tree_score=f.tree_score, d_cost=dc,
                    marginals=mg, anc_states=an)

    fused = G.protocol(device, r0_fused, lambda run: G.sankoff_fwd_bwd(
        run, plan, leaves, cost, L, Q, tau, dts, workspace_bytes=wsb))
    G.assert_bitwise(fused["dp"], dp, "dp: fused vs forward")

    G.protocol(device, lambda: dict(anc_states=eng.backtrack(c, dp_dev)),
               lambda run: G.sankoff_backtrack(run, plan, cost, dp, L, Q))
    G.protocol(device, lambda: dict(trex_dp=eng.to_trex_layout(dp_dev, lv)),
               lambda run: G.dp_to_trex_layout(run, plan, dp, leaves, L, Q))
    took = lib().trex_debug_site2_launches() - site2_before
    assert (took > 0) == (fam == "q20-site2"), took


def test_persistent_forward_second_item_per_wave(device, monkeypatch):
    """Q = 4 lane-per-site forward with more items than co-resident waves (a CU
    holds at most 32 one-wave workgroups): some waves loop and prefetch the
    next item's leaf tile (L = 68: the dword prefetch)."""
    _env(monkeypatch, _LANE)
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    Q, n, L = 4, 4, 68
    B = 32 * cus + 8
    assert B * 2 > 64 * cus
    ch, leaves, cost, _ = inputs(Q, n, L, False, B=B)
    plan = TreePlan(ch)
    eng = SankoffEngine(plan, L, Q, device)
    lv, c = _dev(leaves, device), _dev(cost, device)

    def r0():
        f = eng.forward(lv, c, 0.0, site_score=True)
        return dict(dp=f.dp, site_score=f.site_score, tree_score=f.tree_score)

    G.protocol(device, r0, lambda run: G.sankoff_fwd(run, plan, leaves, cost, L, Q, 0.0))


# ---------------------------------------------------------------------------
# outside, NNI and attachment scores
# ---------------------------------------------------------------------------
NNI = [(Q, tau, n, L) for Q in (2, 3, 4, 5, 20) for tau in (0.0, 0.5)
       for n, L in ((3, 1), (5, 67), (9, 68))]


@pytest.mark.parametrize("Q,tau,n,L", NNI, ids=[f"q{c[0]}-{c[1]}-{c[2]}x{c[3]}" for c in NNI])
def test_outside_nni_attach(device, monkeypatch, Q, tau, n, L):
    _env(monkeypatch, {})
    ch, leaves, cost, _ = inputs(Q, n, L, tau > 0.0)
    plan = TreePlan(ch)
    eng = SankoffEngine(plan, L, Q, device)
    lv, c = _dev(leaves, device), _dev(cost, device)
    dp_dev = eng.forward(lv, c, tau).dp
    dp = dp_dev.cpu()
    outside = G.protocol(device, lambda: dict(outside=eng.outside(lv, c, tau, dp_dev)),
                         lambda run: G.sankoff_outside(run, plan, leaves, cost, L, Q, tau, dp)
                         )["outside"]
    out_dev = outside.to(device)
    G.protocol(device,
               lambda: dict(nni_score=eng.nni_scores(lv, c, tau, dp=dp_dev, outside=out_dev)),
               lambda run: G.sankoff_nni(run, plan, leaves, cost, L, Q, tau, dp, outside))
    new_leaf = random_leaves(plan.B, 1, L, Q, seed=Q + L, missing=0.05)[:, 0]
    sub_rows = np.ascontiguousarray(dp.numpy()[:, -1])  # a subtree's root DP rows (B, L, Q)
    nl_dev, sr_dev = _dev(new_leaf, device), _dev(sub_rows, device)
    G.protocol(device, lambda: dict(attach_score=eng.attach_scores(
        lv, c, tau, new_leaf=nl_dev, dp=dp_dev, outside=out_dev)),
        lambda run: G.sankoff_attach(run, plan, leaves, cost, L, Q, tau, dp, outside,
                                     new_leaf=new_leaf))
    G.protocol(device, lambda: dict(attach_score=eng.attach_scores(
        lv, c, tau, sub_rows=sr_dev, dp=dp_dev, outside=out_dev)),
        lambda run: G.sankoff_attach(run, plan, leaves, cost, L, Q, tau, dp, outside,
                                     sub_rows=sub_rows))


# ---------------------------------------------------------------------------
# ragged batches
# ---------------------------------------------------------------------------
# (n_leaves, L) of tests/test_ragged_gpu.py's SIZES: L covers 1, 64, 65, 130
SIZES = [(5, 100), (9, 64), (32, 130), (2, 1), (17, 1000), (3, 65)]

RAGGED = [(Q, tau) for Q in (4, 20, 61, 100) for tau in (0.0, 0.5)]


@pytest.mark.parametrize("Q,tau", RAGGED, ids=[f"q{q}-{t}" for q, t in RAGGED])
def test_ragged(device, monkeypatch, Q, tau):
    _env(monkeypatch, {})
    chs = [random_topologies(1, n, seed=Q + i)[0] for i, (n, _) in enumerate(SIZES)]
    lvs = [random_leaves(1, n, L, Q, seed=Q + 10 + i, missing=0.05)[0]
           for i, (n, L) in enumerate(SIZES)]
    plan = RaggedTreePlan(chs, [L for _, L in SIZES])
    leaves = plan.pack_leaves(lvs)
    assert leaves.size % 4 != 0  # the packed codes end off a dword
    cost = general_cost(Q, 1, "asym_frac" if tau > 0.0 else "asym_int")
    dts = np.linspace(0.5, 2.0, plan.B).astype(np.float32)
    eng = RaggedSankoffEngine(plan, Q, device)
    lv, c, d = _dev(leaves, device), _dev(cost, device), _dev(dts, device)

    def r0_fwd():
        ts, dp, ss = eng.forward(lv, c, tau, site_score=True)
        return dict(tree_score=ts, dp=dp, site_score=ss)

    dp = G.protocol(device, r0_fwd,
                    lambda run: G.sankoff_ragged(run, 1, plan, leaves, cost, Q, tau))["dp"]
    dp_dev = dp.to(device)

    def r0_bwd():
        dc, mg, an = eng.backward(lv, c, tau, dp_dev, d, marginals=True, anc_states=True)
        return dict(d_cost=dc, marginals=mg, anc_states=an)

    G.protocol(device, r0_bwd, lambda run: G.sankoff_ragged(run, 2, plan, leaves, cost, Q, tau,
                                                            dp=dp, d_tree_score=dts))

    def r0_fused():
        ts, dp3, ss, dc, mg, an = eng.fwd_bwd(lv, c, tau, d, site_score=True, marginals=True,
                                              anc_states=True)
        return dict(tree_score=ts, dp=dp3, site_score=ss, d_cost=dc, marginals=mg, anc_states=an)

    G.protocol(device, r0_fused, lambda run: G.sankoff_ragged(run, 3, plan, leaves, cost, Q, tau,
                                                              d_tree_score=dts))
    G.protocol(device, lambda: dict(anc_states=eng.backtrack(c, dp_dev)),
               lambda run: G.sankoff_ragged_backtrack(run, plan, cost, dp, Q))


# ---------------------------------------------------------------------------
# raw-table path: in/out tables keep the caller's bytes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [4, 130], ids=["q4", "q130"])
def test_raw_tables(device, Q):
    n, L = 5, 67
    n_all = 2 * n - 1
    rng = np.random.default_rng(Q)
    ch = random_topologies(1, n, seed=Q)
    adj = adjacency_from_children(ch)[0]
    children = np.ascontiguousarray(children_from_adjacency(adj, drop_root_self_loop=False)[0],
                                    dtype=np.int32)
    seqs = rng.integers(0, Q, size=(n, L)).astype(np.float32)
    cost = general_cost(Q, 1, "asym_int")
    # caller-chosen tables: what run_dp does not write must come back as given
    dp0 = rng.integers(0, 9, size=(L, n_all, Q)).astype(np.float32)
    bt0 = rng.integers(-3, 5, size=(L, n_all, Q, 4)).astype(np.float32)

    def r0_dp():
        dp, bt = vectorized_dp(adj, dp0, bt0, seqs, cost, device=device)
        return dict(dp=dp, bt=bt)

    tabs = G.protocol(device, r0_dp, lambda run: G.run_dp(
        run, children, np.ascontiguousarray(seqs[:, None, :]), cost, dp0, bt0))
    dp, bt = tabs["dp"], tabs["bt"]
    # leaf rows keep the caller's values except the leaf's own state
    keep = np.ones((L, n, Q), bool)
    keep[np.arange(L)[:, None], np.arange(n)[None, :], seqs.T.astype(np.int64)] = False
    assert np.array_equal(dp.numpy()[:, :n][keep], dp0[:, :n][keep])
    assert np.array_equal(bt.numpy()[:, :n], bt0[:, :n])

    dp_dev, bt_dev = dp.to(device), bt.to(device)
    G.protocol(device, lambda: dict(states=vmapped_backtrack(n_all - 1, None, bt_dev, n_all, n,
                                                             dp=dp_dev)),
               lambda run: G.backtrack_generic(run, n_all - 1, dp, bt, n))

    def r0_total():
        site_min = torch.empty(L, dtype=torch.float32, device=device)
        total = torch.empty(1, dtype=torch.float32, device=device)
        check(lib().trex_dp_root_total(ptr(dp_dev), L, n_all, Q, ptr(site_min), ptr(total),
                                       stream_handle(device)))
        return dict(site_min=site_min, total=total)

    tot = G.protocol(device, r0_total, lambda run: G.dp_root_total(run, dp))
    assert float(tot["total"]) == np.float32(dp.numpy()[:, -1].min(axis=1).astype(np.float64).sum())


# ---------------------------------------------------------------------------
# captured replay of the families test_repeated_launches_reset_reduction_counters
# does not capture: a launch off the caller's stream is an error under capture
# ---------------------------------------------------------------------------
def _capture(fn):
    """fn() warmed up eagerly (plans uploaded, lazy workspaces made), then
    captured once (a linear capture on torch's capture stream) and replayed
    twice: each replay bitwise the eager result."""
    eager = {k: v.clone() for k, v in fn().items()}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    for rep in range(2):
        for v in out.values():
            v.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in eager:
            G.assert_bitwise(out[k], eager[k], f"{k}: replay {rep} vs eager")


def _fused_fn(device, Q):
    n, L, tau = 9, 68, 0.5
    ch, leaves, cost, dts = inputs(Q, n, L, True)
    eng = SankoffEngine(TreePlan(ch), L, Q, device)
    lv, c, d = _dev(leaves, device), _dev(cost, device), _dev(dts, device)

    def fn():
        f, dc, mg, an = eng.fwd_bwd(lv, c, tau, d, site_score=True, marginals=True,
                                    anc_states=True)
        return dict(dp=f.dp, site_score=f.site_score, tree_score=f.tree_score, d_cost=dc,
                    marginals=mg, anc_states=an)
    return fn


def _nni_fn(device):
    Q, n, L, tau = 4, 9, 68, 0.5
    ch, leaves, cost, _ = inputs(Q, n, L, True)
    eng = SankoffEngine(TreePlan(ch), L, Q, device)
    lv, c = _dev(leaves, device), _dev(cost, device)
    new_leaf = _dev(random_leaves(3, 1, L, Q, seed=3)[:, 0], device)
    dp = eng.forward(lv, c, tau).dp

    def fn():
        outside = eng.outside(lv, c, tau, dp)
        return dict(outside=outside,
                    nni_score=eng.nni_scores(lv, c, tau, dp=dp, outside=outside),
                    attach_score=eng.attach_scores(lv, c, tau, new_leaf=new_leaf, dp=dp,
                                                   outside=outside))
    return fn


def _ragged_fn(device):
    Q, tau = 4, 0.5
    sizes = [(9, 68)] * 3
    chs = [random_topologies(1, n, seed=40 + i)[0] for i, (n, _) in enumerate(sizes)]
    lvs = [random_leaves(1, n, L, Q, seed=50 + i, missing=0.05)[0]
           for i, (n, L) in enumerate(sizes)]
    plan = RaggedTreePlan(chs, [L for _, L in sizes])
    eng = RaggedSankoffEngine(plan, Q, device)
    lv = _dev(plan.pack_leaves(lvs), device)
    c = _dev(general_cost(Q, 1, "asym_frac"), device)
    d = _dev(np.linspace(0.5, 2.0, 3).astype(np.float32), device)

    def fn():
        ts, dp, ss, dc, mg, an = eng.fwd_bwd(lv, c, tau, d, site_score=True, marginals=True,
                                             anc_states=True)
        return dict(tree_score=ts, dp=dp, site_score=ss, d_cost=dc, marginals=mg, anc_states=an)
    return fn


CAPTURES = {
    "fused-q20-site": lambda dev: _fused_fn(dev, 20),  # three launches: gate, site, reduce
    "fused-q21": lambda dev: _fused_fn(dev, 21),
    "fused-q100": lambda dev: _fused_fn(dev, 100),
    "outside-nni-attach-q4": _nni_fn,
    "ragged-fused-q4": _ragged_fn,
}


@pytest.mark.parametrize("what", list(CAPTURES))
def test_captured_replay(device, monkeypatch, what):
    """n = 9, L = 68, B = 3, tau = 0.5, nothing set in the environment."""
    _env(monkeypatch, {})
    _capture(CAPTURES[what](device))
