"""The guard-band harness (tests/_guard.py) catches what it claims, on CPU
tensors: stand-in "kernels" written as torch ops on the guarded allocation --
the only deliberately wrong code of the guard tests -- must each be flagged
with the offset or entry at fault, and a well-behaved one must pass.
tests/test_guard_gpu.py repeats the first and the third on the device.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from _guard import GUARD_BYTES, PROTOCOL, Run, assert_bitwise, guarded, protocol

CPU = torch.device("cpu")
N = 67  # odd: the int8 payload ends off every alignment


def _x():
    return (np.arange(N) % 4).astype(np.int8)


def _good(run, x):
    """out[i] = 2 x[i] + 1, every entry written, nothing else touched."""
    xi = run.input("x", x)
    out = run.output("out", (N,), torch.float32)
    out.copy_(2.0 * xi.to(torch.float32) + 1.0)
    return xi, out


def _r0():
    return {"out": torch.from_numpy(2.0 * _x().astype(np.float32) + 1.0)}


def test_layout_and_fill_bytes():
    v, h = guarded((3, N), torch.int8, CPU, payload=np.ones((3, N), np.int8), guard_byte=0x5A)
    assert h.flat.numel() == 2 * GUARD_BYTES + 3 * N and h.nbytes == 3 * N
    assert v.data_ptr() == h.flat.data_ptr() + GUARD_BYTES and v.data_ptr() % 16 == 0
    assert bool((h.flat[:GUARD_BYTES] == 0x5A).all())
    assert bool((h.flat[GUARD_BYTES + 3 * N:] == 0x5A).all())  # starts at the byte after
    assert h.flat[GUARD_BYTES + 3 * N:].numel() == GUARD_BYTES
    assert bool((v == 1).all())
    h.check()
    h.unchanged()
    f, hf = guarded((5,), torch.float32, CPU, payload=0xFF, guard_byte=0xA5)
    assert bool(torch.isnan(f).all())  # the R2 prefill reads as NaN
    assert PROTOCOL[1] == dict(in_guard=0x01, prefill=0x00, out_guard=0xA5)
    assert PROTOCOL[2] == dict(in_guard=0xFF, prefill=0xFF, out_guard=0x5A)


def test_well_behaved_stand_in_passes():
    out = protocol(CPU, _r0, lambda run: _good(run, _x()))
    assert_bitwise(out["out"], _r0()["out"], "out")


def test_store_one_past_the_payload_is_flagged():
    def call(run):
        _good(run, _x())
        h = run.outputs["out"]
        h.flat[GUARD_BYTES + h.nbytes] = 0
    with pytest.raises(AssertionError, match=rf"output out.*first at offset {4 * N}, last at "
                                             rf"offset {4 * N} "):
        protocol(CPU, _r0, call)


def test_store_one_before_the_payload_is_flagged():
    def call(run):
        _good(run, _x())
        run.outputs["out"].flat[GUARD_BYTES - 1] = 0
    with pytest.raises(AssertionError, match=r"output out.*first at offset -1, last at offset -1 "):
        protocol(CPU, _r0, call)


def test_store_past_a_workspace_reports_how_far_it_reached():
    def call(run):
        _good(run, _x())
        run.workspace(100)
        h = run.scratch["workspace"]
        h.flat[GUARD_BYTES + 100:GUARD_BYTES + 132] = 7
    with pytest.raises(AssertionError, match=r"workspace workspace: 32 guard byte.*first at offset "
                                             r"100, last at offset 131 "):
        protocol(CPU, _r0, call)


def test_last_entry_left_unwritten_is_flagged():
    def call(run):
        xi = run.input("x", _x())
        out = run.output("out", (N,), torch.float32)
        out[:N - 1].copy_(2.0 * xi[:N - 1].to(torch.float32) + 1.0)
    with pytest.raises(AssertionError, match=rf"out: R1 vs R2.*1 of {N} entries differ, first at "
                                             rf"flat index {N - 1} "):
        protocol(CPU, _r0, call)


def test_result_that_depends_on_the_guard_after_an_input_is_flagged():
    def call(run):
        xi, out = _good(run, _x())
        h = run.inputs["x"]
        out[3] += h.flat[GUARD_BYTES + h.nbytes].to(torch.float32)  # x[N], one past the input
    with pytest.raises(AssertionError, match=rf"out: R1 vs R2.*1 of {N} entries differ, first at "
                                             r"flat index 3 "):
        protocol(CPU, _r0, call)


def test_input_element_overwritten_is_flagged():
    def call(run):
        xi, _ = _good(run, _x())
        xi[5] = 3 - xi[5]
    with pytest.raises(AssertionError, match=rf"input x: input overwritten: 1 byte.*first in "
                                             rf"element 5, last in element 5 of {N}"):
        protocol(CPU, _r0, call)


def test_in_out_table_keeps_the_callers_bytes():
    """An in/out table (trex_run_dp's dp / bt): the entries the call leaves
    alone hold the caller's values in both runs, so R1 == R2 and == R0."""
    t0 = np.arange(12, dtype=np.float32).reshape(3, 4)

    def call(run):
        t = run.inout("t", t0)
        t[1] = -1.0

    want = torch.from_numpy(t0.copy())
    want[1] = -1.0
    protocol(CPU, lambda: {"t": want}, call)


def test_r0_mismatch_is_flagged():
    with pytest.raises(AssertionError, match="out: R1 vs R0"):
        protocol(CPU, lambda: {"out": _r0()["out"] + 1.0}, lambda run: _good(run, _x()))


def test_run_names_are_unique():
    run = Run(CPU, 1)
    run.input("x", _x())
    with pytest.raises(AssertionError):
        run.output("x", (N,), torch.float32)


# ---------------------------------------------------------------------------
# kept regions (trex_tree_gram_skip's cached block, the root row of
# trex_datagen_nk_tree's seqs, padding that is the caller's to zero)
# ---------------------------------------------------------------------------
KEEP = np.zeros(N, bool)
KEEP[:8] = True  # the call leaves out[0..8) alone


def _kept(run, x, upto=N):
    """out[i] = 2 x[i] + 1 for 8 <= i < upto."""
    xi = run.input("x", x)
    out = run.output("out", (N,), torch.float32, keep=KEEP)
    out[8:upto].copy_(2.0 * xi[8:upto].to(torch.float32) + 1.0)
    return xi, out


def test_kept_region_holds_each_runs_prefill_and_is_not_compared():
    """R1's kept bytes are 0x00 and R2's 0xFF -- they differ, and R0's hold
    whatever the method left there: none of it is compared."""
    out = protocol(CPU, lambda: {"out": _r0()["out"] + torch.from_numpy(KEEP * 9.0).float()},
                   lambda run: _kept(run, _x()))
    assert bool((out["out"][:8] == 0).all())
    assert_bitwise(out["out"][8:], _r0()["out"][8:], "out")


def test_write_into_the_kept_region_is_flagged():
    def call(run):
        _, out = _kept(run, _x())
        out[7] = 1.0  # the same value in both runs: R1 == R2 alone would pass
    with pytest.raises(AssertionError, match=rf"R1 output out: kept region written: 1 of 8 kept "
                                             rf"entries changed, first at flat index 7, last at 7 "
                                             rf"of {N}"):
        protocol(CPU, _r0, call)


def test_entry_outside_the_kept_region_left_unwritten_is_flagged():
    with pytest.raises(AssertionError, match=rf"out: R1 vs R2.*1 of {N} entries differ, first at "
                                             rf"flat index {N - 1} "):
        protocol(CPU, _r0, lambda run: _kept(run, _x(), upto=N - 1))


def test_kept_padding_prefilled_by_the_caller_must_stay_as_filled():
    """fill=: the kept entries hold the caller's value (the zeros a header
    asks the caller for) in both runs; a call that relies on them may read
    them, and one that writes them is flagged."""
    def call(run, spoil):
        xi = run.input("x", _x())
        out = run.output("out", (N,), torch.float32, keep=KEEP, fill=0.0)
        assert bool((out[:8] == 0).all())
        out[8:].copy_(2.0 * xi[8:].to(torch.float32) + 1.0 + out[:8].sum())
        if spoil:
            out[0] = 2.0
    protocol(CPU, _r0, lambda run: call(run, False))
    with pytest.raises(AssertionError, match="kept region written: 1 of 8"):
        protocol(CPU, _r0, lambda run: call(run, True))


def test_in_out_table_with_a_kept_row():
    """trex_datagen_nk_tree's seqs: the root row is the caller's and stays."""
    t0 = np.arange(12, dtype=np.int8).reshape(3, 4)
    keep = np.zeros((3, 4), bool)
    keep[2] = True

    def call(run, spoil):
        t = run.inout("t", t0, keep=keep)
        t[:2] = 5
        if spoil:
            t[2, 1] = t0[2, 1] + 1

    want = torch.from_numpy(t0.copy())
    want[:2] = 5
    protocol(CPU, lambda: {"t": want}, lambda run: call(run, False))
    with pytest.raises(AssertionError, match=r"output t: kept region written: 1 of 4 kept entries "
                                             r"changed, first at flat index 9, last at 9 of 12"):
        protocol(CPU, lambda: {"t": want}, lambda run: call(run, True))
