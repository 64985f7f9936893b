"""Guard-band tests of the per-branch change entry points:
trex_sankoff_edge_changes_w and trex_sankoff_sets_edge_changes_w stay inside
their buffers.

The three-run protocol of tests/_guard.py (R0 on the engine method's own
buffers, R1 and R2 through the C ABI between 1 MiB canaries with different
guard and prefill bytes; R1 == R2 == R0 bitwise, every guard intact, every
input unchanged) at (n, L, Q) = (6, 70, 4) and (7, 33, 5), tau = 0 and 0.5,
with and without weights.  The last tile has 6 / 33 live lanes: the tail lanes
read the last site's states and weight and store nothing.  The workspace is
exactly trex_edge_workspace_bytes bytes and is prefilled like an output (0x00
in R1, 0xFF -- NaN partials -- in R2), so a count that depends on what the
partials held, or the root's entries if they were read from them, shows as
R1 != R2.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import _guard as G
from test_nni_gpu import case as nni_case
from trex_amd import SankoffEngine, TreePlan, sets_from_codes

pytestmark = pytest.mark.gpu

F32 = torch.float32


def _dev(x, device):
    return torch.as_tensor(np.ascontiguousarray(x)).to(device).contiguous()


def edges(run, fn_name, plan, leaves, cost, L, Q, tau, dp, outside, states, weights):
    check, lib, ptr, st = G._abi(run.device)
    pl, lv, c = run.input("attach_plan", plan.attach_host), run.input("leaves", leaves), \
        run.input("cost", cost)
    dpt, ot = run.input("dp", dp), run.input("outside", outside)
    sd, w = run.input("states", states), run.input("weights", weights)
    counts = run.output("counts", (plan.B, plan.n_all, Q, Q), F32)
    lengths = run.output("lengths", (plan.B, plan.n_all), F32)
    lmin = lmax = None
    if tau == 0.0:
        lmin = run.output("length_min", (plan.B, plan.n_all), F32)
        lmax = run.output("length_max", (plan.B, plan.n_all), F32)
    nb = int(lib.trex_edge_workspace_bytes(plan.B, L, plan.n_all, Q))
    assert nb == plan.B * ((L + 63) // 64) * plan.n_all * (Q * Q + 2) * 8
    ws = run.workspace(nb)
    check(getattr(lib, fn_name)(ptr(pl), ptr(lv), ptr(c), plan.B, L, plan.n_all, Q, float(tau),
                                ptr(dpt), ptr(ot), ptr(sd), ptr(w), ptr(counts), ptr(lengths),
                                ptr(lmin), ptr(lmax), ptr(ws), nb, st))


@pytest.mark.parametrize("tau", [0.0, 0.5])
@pytest.mark.parametrize("n,L,Q", [(6, 70, 4), (7, 33, 5)])
def test_edge_entry_points_stay_inside_their_buffers(device, n, L, Q, tau):
    ch, codes, cost, _ = nni_case(n, L, Q, tau)
    plan = TreePlan(ch)
    eng = SankoffEngine(plan, L, Q, device)
    c = _dev(cost, device)
    w = np.random.default_rng(n + L).uniform(0.25, 2.0, size=(3, L)).astype(np.float32)
    wd = _dev(w, device)
    for fn_name, leaves in (("trex_sankoff_edge_changes_w", codes),
                            ("trex_sankoff_sets_edge_changes_w", sets_from_codes(codes, Q))):
        lv = _dev(leaves, device)
        f = eng.forward(lv, c, tau)
        out = eng.outside(lv, c, tau, f.dp)
        states = eng.backtrack(c, f.dp) if tau == 0.0 else None
        dp_h, out_h = f.dp.cpu().numpy(), out.cpu().numpy()
        st_h = None if states is None else states.cpu().numpy()
        for wh, wt in ((None, None), (w, wd)):
            got = G.protocol(device, lambda: vars(eng.edge_changes(
                lv, c, tau, dp=f.dp, outside=out, states=states, weights=wt)),
                lambda run: edges(run, fn_name, plan, leaves, cost, L, Q, tau, dp_h, out_h, st_h,
                                  wh))
            assert set(got) == ({"counts", "lengths", "length_min", "length_max"} if tau == 0.0
                                else {"counts", "lengths"})
            # every site is on every one of the 2 n - 2 edges with its whole weight
            total = (float(w.sum()) if wh is not None else 3.0 * L) * (2 * n - 2)
            assert abs(float(got["counts"].double().sum()) - total) <= 1e-4 * total
            assert not got["counts"][:, -1].any()
