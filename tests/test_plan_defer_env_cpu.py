"""TREX_DEFER is read at every plan build (plan.cpp), not once per process:
one process can build the deferred and the undeferred plan of the same trees,
which is what the GPU A/B tests of the deferred-cherry path rely on."""

from __future__ import annotations

from _cases import random_topologies
from trex_amd import TreePlan

K_STEP_DEFERRED_IN = 8  # trex_common.h


def _n_deferred(plan):
    return int(((plan.fwd_steps[:, :, 3] & K_STEP_DEFERRED_IN) != 0).sum())


def test_trex_defer_is_read_per_plan_build(monkeypatch):
    ch = random_topologies(2, 16, seed=1)
    monkeypatch.setenv("TREX_DEFER", "0")
    assert _n_deferred(TreePlan(ch)) == 0
    monkeypatch.delenv("TREX_DEFER")
    assert _n_deferred(TreePlan(ch)) >= 1
    monkeypatch.setenv("TREX_DEFER", "0")
    assert _n_deferred(TreePlan(ch)) == 0
