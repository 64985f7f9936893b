"""The fused Q = 4 program (trex_fused4_program_build, plan.cpp; layout:
trex_common.h) against the plan's forward steps it was decoded from.

The program is a header of 16 ints {magic 'TRF4', B, n_all, n_int} and one
record of 8 ints per forward step, tree by tree in the plan's order:
[flags | forward class << 16, row, operand 0, operand 1,
own slot * 1024, re-read row 0, re-read row 1, 0].  Every field is checked
against TreePlan.fwd_steps; the plan itself must come back unchanged.
"""

from __future__ import annotations

import numpy as np
import pytest

from _cases import balanced_children, random_topologies, weird_children
from trex_amd import TreePlan
from trex_amd._lib import TREX_E_UNSUPPORTED, TREX_OK, TREX_PLAN_HEADER_INTS, lib

MAGIC = 0x54524634
LEAF, PREV, DEFER = (1, 2), (4, 8), (16, 32)
DEFER_IN, TO_NEXT, ROOT, PUT = 64, 128, 256, 512
CHERRY, CHERRY_DEFERRED, LEAF_INT, INT_INT = range(4)
# the plan's own bits (trex_common.h)
ACCUMULATE, CHILD_PREV, CHILD_DEFERRED = 1 << 26, 1 << 27, 1 << 28
STEP_ROOT, STEP_UNREACHED, STEP_TO_NEXT, STEP_DEFERRED_IN = 1, 2, 4, 8


def pectinate(n):
    ch = np.full((2 * n - 1, 2), -1, dtype=np.int32)
    ch[n] = (0, 1)
    for k in range(1, n - 1):
        ch[n + k] = (k + 1, n + k - 1)
    return ch[None]


def build(plan):
    n = lib().trex_fused4_program_ints(plan.B, plan.n_all)
    assert n == TREX_PLAN_HEADER_INTS + plan.B * plan.n_int * 8
    prog = np.full(n, -7, dtype=np.int32)
    rc = lib().trex_fused4_program_build(plan.host.ctypes.data, plan.B, plan.n_all,
                                         prog.ctypes.data)
    return rc, prog


TREES = {
    "random8": lambda: random_topologies(3, 8, seed=1),
    "random13": lambda: random_topologies(3, 13, seed=2),
    "random32": lambda: random_topologies(4, 32, seed=3),
    "balanced16": lambda: balanced_children(16, B=2),
    "pectinate16": lambda: pectinate(16),
}


@pytest.mark.parametrize("defer", ["0", "1"])
@pytest.mark.parametrize("kind", list(TREES))
def test_program_matches_the_plans_steps(monkeypatch, kind, defer):
    monkeypatch.setenv("TREX_DEFER", defer)
    plan = TreePlan(TREES[kind]())
    before, word = plan.host.copy(), plan.slot_word
    rc, prog = build(plan)
    assert rc == TREX_OK, lib().trex_last_error()
    assert np.array_equal(plan.host, before) and plan.slot_word == word
    assert list(prog[:4]) == [MAGIC, plan.B, plan.n_all, plan.n_int]
    assert not prog[4:TREX_PLAN_HEADER_INTS].any()
    rec = prog[TREX_PLAN_HEADER_INTS:].reshape(plan.B, plan.n_int, 8)
    steps = plan.fwd_steps
    n_deferred = 0
    for b in range(plan.B):
        for k in range(plan.n_int):
            e, r = [int(x) for x in steps[b, k]], [int(x) for x in rec[b, k]]
            fl = r[0] & 0xFFFF
            assert r[1] == e[0] & 0xFFFF and r[7] == 0
            leaf = []
            for c in (0, 1):
                d = e[1 + c]
                kind_c = (d >> 24) & 3
                assert kind_c in (1, 2) and not d & ACCUMULATE
                leaf.append(kind_c == 1)
                assert bool(fl & LEAF[c]) == leaf[c]
                if leaf[c]:
                    assert r[2 + c] == (d & 0xFFFF) * 64 and (d & 0xFFFF) < plan.n_leaves
                    assert r[5 + c] == -1 and not fl & (PREV[c] | DEFER[c])
                else:
                    prev, deferred = bool(d & CHILD_PREV), bool(d & CHILD_DEFERRED)
                    assert bool(fl & PREV[c]) == prev and bool(fl & DEFER[c]) == deferred
                    slot = (d >> 16) & 0xFF
                    assert r[2 + c] == (0 if prev else slot * 1024)
                    assert prev or slot < plan.n_slots
                    assert r[5 + c] == (-1 if deferred else d & 0xFFFF)
                    if prev:  # the bypassed child is the step before
                        assert k > 0 and steps[b, k - 1, 0] & 0xFFFF == d & 0xFFFF
                        assert steps[b, k - 1, 3] & STEP_TO_NEXT
            assert not e[3] & STEP_UNREACHED
            assert bool(fl & DEFER_IN) == bool(e[3] & STEP_DEFERRED_IN)
            assert bool(fl & TO_NEXT) == bool(e[3] & STEP_TO_NEXT)
            assert bool(fl & ROOT) == bool(e[3] & STEP_ROOT) == (k == plan.n_int - 1)
            oslot = (e[0] >> 16) & 0xFF
            put = not e[3] & STEP_TO_NEXT and oslot != 0xFF
            assert bool(fl & PUT) == put and r[4] == (oslot * 1024 if put else 0)
            # a reverse step takes its cotangent from the bypass, the root's
            # registers or its own slot
            assert fl & (TO_NEXT | ROOT) or put
            fcls = (CHERRY_DEFERRED if fl & DEFER_IN else CHERRY) if all(leaf) else (
                LEAF_INT if any(leaf) else INT_INT)
            assert r[0] >> 16 == fcls
            n_deferred += bool(fl & DEFER_IN)
    assert (n_deferred > 0) == (defer == "1" and plan.n_int > 1)


@pytest.mark.parametrize("case", ["fwdref", "dag", "cycle"])
def test_sentinel_unreached_and_two_parent_trees_are_refused(case):
    plan = TreePlan(weird_children(case)[None])
    steps = plan.fwd_steps[0]
    kinds = (steps[:, 1:3] >> 24) & 3
    assert ((kinds == 0).any() or (steps[:, 3] & STEP_UNREACHED).any()
            or (steps[:, 1:3] & ACCUMULATE).any())
    rc, _ = build(plan)
    assert rc == TREX_E_UNSUPPORTED
    assert b"trex_fused4_program_build" in lib().trex_last_error()


def test_a_plan_of_another_shape_is_an_argument_error():
    plan = TreePlan(random_topologies(2, 8, seed=4))
    prog = np.zeros(lib().trex_fused4_program_ints(3, plan.n_all), dtype=np.int32)
    rc = lib().trex_fused4_program_build(plan.host.ctypes.data, 3, plan.n_all, prog.ctypes.data)
    assert rc == -1
