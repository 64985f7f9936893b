"""Guard-band tests of the state-set entry points: trex_sankoff_sets_fwd,
_sets_outside, _sets_nni_w and _sets_attach_w stay inside their buffers.

The three-run protocol of tests/_guard.py (R0 on the engine method's own
buffers, R1 and R2 through the C ABI between 1 MiB canaries with different
guard and prefill bytes; R1 == R2 == R0 bitwise, every guard intact, every
input unchanged) at L = 65 with Q = 3 and Q = 5: the int32 masks (B * n * 65
words), the fp32 tables (65 * Q floats per row, 12-byte rows for Q = 3) and the
weights end on odd word counts directly against the back guard, and the last
tile has one live lane and 63 tail lanes.  The workspace is exactly the size
the ``*_workspace_bytes`` function returns and is prefilled like an output.
B = 3 topologies of 5 leaves, tree 1 a caterpillar; masks with empty, full and
ambiguous cells and bits above Q set.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import _guard as G
from _cases import general_cost, random_topologies
from trex_amd import SankoffEngine, TreePlan
from trex_amd._lib import TREX_FLAG_HARD_ROOT

pytestmark = pytest.mark.gpu

F32 = torch.float32
B, N, L = 3, 5, 65


@functools.lru_cache(maxsize=None)
def inputs(Q, soft):
    ch = random_topologies(B, N, seed=7 * N + L)
    ch[1, N] = (0, 1)
    for k in range(1, N - 1):
        ch[1, N + k] = (k + 1, N + k - 1)  # a caterpillar
    rng = np.random.default_rng(100 * Q + L)
    kind = rng.random((B, N + 1, L))
    m = 1 << rng.integers(0, Q, size=kind.shape)
    m = np.where(kind < 0.3, m | rng.integers(0, 1 << Q, size=kind.shape), m)
    m = np.where(kind < 0.1, (1 << Q) - 1, m)
    m = np.where(kind < 0.05, 0, m)
    m = (m | (rng.integers(0, 1 << 11, size=kind.shape) << 20)).astype(np.int32)
    cost = general_cost(Q, 1, "asym_frac" if soft else "asym_int")
    w = rng.uniform(0.25, 2.0, size=(B, L)).astype(np.float32)
    return ch, np.ascontiguousarray(m[:, :N]), np.ascontiguousarray(m[:, N]), cost, w


def _dev(x, device):
    return torch.as_tensor(np.ascontiguousarray(x)).to(device).contiguous()


def sets_fwd(run, plan, masks, cost, Q, tau, flags):
    check, lib, ptr, st = G._abi(run.device)
    pl, lv, c = run.input("attach_plan", plan.attach_host), run.input("leaf_sets", masks), \
        run.input("cost", cost)
    dp = run.output("dp", G._dp_shape(plan, L, Q), F32)
    ss = run.output("site_score", (plan.B, L), F32)
    ts = run.output("tree_score", (plan.B,), F32)
    nb = int(lib.trex_sets_fwd_workspace_bytes(plan.B, L, plan.n_all, Q))
    ws = run.workspace(nb)
    check(lib.trex_sankoff_sets_fwd(ptr(pl), ptr(lv), ptr(c), plan.B, L, plan.n_all, Q, float(tau),
                                    flags, ptr(dp), ptr(ss), ptr(ts), ptr(ws), nb, st))


def sets_outside(run, plan, masks, cost, Q, tau, dp):
    check, lib, ptr, st = G._abi(run.device)
    pl, lv, c = run.input("nni_plan", plan.nni_host), run.input("leaf_sets", masks), \
        run.input("cost", cost)
    dpt = run.input("dp", dp)
    out = run.output("outside", G._dp_shape(plan, L, Q), F32)
    check(lib.trex_sankoff_sets_outside(ptr(pl), ptr(lv), ptr(c), plan.B, L, plan.n_all, Q,
                                        float(tau), ptr(dpt), ptr(out), st))


def sets_nni(run, plan, masks, cost, Q, tau, dp, outside, weights):
    check, lib, ptr, st = G._abi(run.device)
    pl, lv, c = run.input("nni_plan", plan.nni_host), run.input("leaf_sets", masks), \
        run.input("cost", cost)
    dpt, ot, w = run.input("dp", dp), run.input("outside", outside), run.input("weights", weights)
    score = run.output("nni_score", (plan.B, plan.n_int - 1, 2), F32)
    nb = int(lib.trex_nni_workspace_bytes(plan.B, L, plan.n_all, Q))
    ws = run.workspace(nb)
    check(lib.trex_sankoff_sets_nni_w(ptr(pl), ptr(lv), ptr(c), plan.B, L, plan.n_all, Q,
                                      float(tau), ptr(dpt), ptr(ot), ptr(w), ptr(score), ptr(ws),
                                      nb, st))


def sets_attach(run, plan, masks, cost, Q, tau, dp, outside, weights, *, sub_sets=None,
                sub_rows=None):
    check, lib, ptr, st = G._abi(run.device)
    pl, lv, c = run.input("attach_plan", plan.attach_host), run.input("leaf_sets", masks), \
        run.input("cost", cost)
    dpt, ot, w = run.input("dp", dp), run.input("outside", outside), run.input("weights", weights)
    sm, sr = run.input("sub_sets", sub_sets), run.input("sub_rows", sub_rows)
    score = run.output("attach_score", (plan.B, plan.n_all), F32)
    nb = int(lib.trex_attach_workspace_bytes(plan.B, L, plan.n_all, Q))
    ws = run.workspace(nb)
    check(lib.trex_sankoff_sets_attach_w(ptr(pl), ptr(lv), ptr(c), plan.B, L, plan.n_all, Q,
                                         float(tau), ptr(dpt), ptr(ot), ptr(sm), ptr(sr), ptr(w),
                                         ptr(score), ptr(ws), nb, st))


@pytest.mark.parametrize("tau", [0.0, 0.5])
@pytest.mark.parametrize("Q", [3, 5])
def test_sets_entry_points_stay_inside_their_buffers(device, Q, tau):
    ch, masks, new, cost, w = inputs(Q, tau > 0.0)
    plan = TreePlan(ch)
    eng = SankoffEngine(plan, L, Q, device)
    lv, c, wd = _dev(masks, device), _dev(cost, device), _dev(w, device)

    def fwd(hard_root):
        f = eng.forward(lv, c, tau, site_score=True, hard_root=hard_root)
        return dict(dp=f.dp, site_score=f.site_score, tree_score=f.tree_score)

    for hard_root in (False, True):
        flags = TREX_FLAG_HARD_ROOT if hard_root else 0
        dp = G.protocol(device, lambda: fwd(hard_root),
                        lambda run: sets_fwd(run, plan, masks, cost, Q, tau, flags))["dp"]
    dp_dev = dp.to(device)
    outside = G.protocol(device, lambda: dict(outside=eng.outside(lv, c, tau, dp_dev)),
                         lambda run: sets_outside(run, plan, masks, cost, Q, tau, dp))["outside"]
    out_dev = outside.to(device)
    for wh, wt in ((None, None), (w, wd)):
        G.protocol(device, lambda: dict(nni_score=eng.nni_scores(
            lv, c, tau, dp=dp_dev, outside=out_dev, weights=wt)),
            lambda run: sets_nni(run, plan, masks, cost, Q, tau, dp, outside, wh))
        G.protocol(device, lambda: dict(attach_score=eng.attach_scores(
            lv, c, tau, new_leaf=_dev(new, device), dp=dp_dev, outside=out_dev, weights=wt)),
            lambda run: sets_attach(run, plan, masks, cost, Q, tau, dp, outside, wh,
                                    sub_sets=new))
    sub_rows = np.ascontiguousarray(dp.numpy()[:, -1])  # a subtree's root DP rows (B, L, Q)
    G.protocol(device, lambda: dict(attach_score=eng.attach_scores(
        lv, c, tau, sub_rows=_dev(sub_rows, device), dp=dp_dev, outside=out_dev)),
        lambda run: sets_attach(run, plan, masks, cost, Q, tau, dp, outside, None,
                                sub_rows=sub_rows))
