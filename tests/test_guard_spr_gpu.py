"""Guard-band tests of the SPR entry points: trex_sankoff_spr_w and
trex_sankoff_sets_spr_w stay inside their buffers.

The three-run protocol of tests/_guard.py (R0 on the engine method's own
buffers, R1 and R2 through the C ABI between 1 MiB canaries with different
guard and prefill bytes; R1 == R2 == R0 bitwise, every guard intact, every
input unchanged) at (n, L, Q) = (6, 70, 4) and (7, 33, 5), tau = 0 and 0.5,
with and without weights.  The last tile has 6 / 33 live lanes: the tail
lanes store their scratch rows inside the workspace and nowhere else.  The
workspace is exactly trex_spr_workspace_bytes bytes and is prefilled like an
output (0x00 in R1, 0xFF -- NaN rows -- in R2), so a score that depends on what
the scratch rows held, or a +inf entry that is not written, shows as R1 != R2.
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


def spr(run, fn_name, plan, leaves, cost, L, Q, tau, dp, outside, weights):
    check, lib, ptr, st = G._abi(run.device)
    pl, lv, c = run.input("spr_plan", plan.spr_host), run.input("leaves", leaves), \
        run.input("cost", cost)
    dpt, ot, w = run.input("dp", dp), run.input("outside", outside), run.input("weights", weights)
    score = run.output("spr_score", (plan.B, plan.n_all - 1, plan.n_all), F32)
    nb = int(lib.trex_spr_workspace_bytes(plan.B, L, plan.n_all, Q))
    assert nb > 0
    ws = run.workspace(nb)
    check(getattr(lib, fn_name)(ptr(pl), ptr(lv), ptr(c), plan.B, L, plan.n_all, Q, float(tau),
                                ptr(dpt), ptr(ot), ptr(w), ptr(score), ptr(ws), nb, st))


@pytest.mark.parametrize("tau", [0.0, 0.5])
@pytest.mark.parametrize("n,L,Q", [(6, 70, 4), (7, 33, 5)])
def test_spr_entry_points_stay_inside_their_buffers(device, n, L, Q, tau):
    ch, codes, cost, _ = nni_case(n, L, Q, tau)
    plan = TreePlan(ch)
    eng = SankoffEngine(plan, L, Q, device)
    c = _dev(cost, device)
    w = np.random.default_rng(n + L).uniform(0.25, 2.0, size=(3, L)).astype(np.float32)
    wd = _dev(w, device)
    for fn_name, leaves in (("trex_sankoff_spr_w", codes),
                            ("trex_sankoff_sets_spr_w", sets_from_codes(codes, Q))):
        lv = _dev(leaves, device)
        f = eng.forward(lv, c, tau)
        out = eng.outside(lv, c, tau, f.dp)
        dp_h, out_h = f.dp.cpu().numpy(), out.cpu().numpy()
        for wh, wt in ((None, None), (w, wd)):
            got = G.protocol(device, lambda: dict(spr_score=eng.spr_scores(
                lv, c, tau, dp=f.dp, outside=out, weights=wt)),
                lambda run: spr(run, fn_name, plan, leaves, cost, L, Q, tau, dp_h, out_h, wh))
            assert torch.isinf(got["spr_score"]).any() and torch.isfinite(got["spr_score"]).any()
