"""Host checks of the Sankoff dispatch path, callable without a GPU.

Pins the return code and a key word of trex_last_error() for the checks
between an entry point and its kernel launch: the argument checks of
run_phase / trex_sankoff_ragged and the per-family LDS checks behind the
routing.  As in test_args_cpu.py every call is rejected before any launch, so
host numpy buffers stand in for device pointers; the routing knobs are set so
that no case reaches a device query either.
"""

from __future__ import annotations

import numpy as np
import pytest

from trex_amd._lib import TREX_E_ARG, TREX_E_UNSUPPORTED, lib

B, L_SITES, N_ALL = 1, 64, 7
N_INT = N_ALL - (N_ALL + 1) // 2


def _buf(n=1 << 16):
    return np.zeros(n, np.uint8)


def _ws(Q):
    return int(lib().trex_workspace_bytes(B, L_SITES, N_ALL, Q))


def _fwd(Q, *, plan=True, n_slots=2, tau=0.5, flags=0, tree_score=True, ws_bytes=None):
    """trex_sankoff_fwd at the fixed shape -> (rc, last error)."""
    lb = lib()
    b = _buf()
    p = b.ctypes.data
    full = _ws(Q)
    w = _buf(max(full, 1))
    rc = lb.trex_sankoff_fwd(p if plan else None, n_slots, p, p, B, L_SITES, N_ALL, Q, tau, flags,
                             p, None, p if tree_score else None, w.ctypes.data,
                             full if ws_bytes is None else ws_bytes, None)
    return rc, lb.trex_last_error()


def _ragged(Q=4, *, phase=1, items=1, ws_short=0):
    lb = lib()
    b = _buf()
    p = b.ctypes.data
    full = int(lb.trex_ragged_workspace_bytes(max(items, 1), Q))
    w = _buf(full)
    rc = lb.trex_sankoff_ragged(phase, p, B, 2, 4, items, p, p, Q, 0.5, 0, p, None, p, None, p,
                                None, None, w.ctypes.data, full - ws_short, None)
    return rc, lb.trex_last_error()


def test_null_plan():
    rc, err = _fwd(4, plan=False)
    assert rc == TREX_E_ARG, rc
    assert b"null pointer" in err


def test_phase1_needs_tree_score():
    rc, err = _fwd(4, tree_score=False)
    assert rc == TREX_E_ARG, rc
    assert b"tree_score" in err


def test_phase2_needs_d_cost():
    lb = lib()
    b = _buf()
    p = b.ctypes.data
    ws = _ws(4)
    w = _buf(ws)
    rc = lb.trex_sankoff_bwd(p, 2, p, p, B, L_SITES, N_ALL, 4, 0.5, 0, p, None, None, None, None,
                             w.ctypes.data, ws, None)
    assert rc == TREX_E_ARG, rc
    assert b"d_cost" in lb.trex_last_error()


def test_workspace_one_byte_short_q4():
    rc, err = _fwd(4, ws_bytes=_ws(4) - 1)
    assert rc == TREX_E_ARG, rc
    assert b"workspace too small" in err


def test_workspace_q20_kept_rows_are_optional():
    """4 < Q <= 20: a workspace without the site kernel's kept s rows
    (trex_workspace_bytes - B n_int L Q 4 bytes) passes the size
    check -- the call is then refused on the next check, its flags -- and one
    byte less does not."""
    srow_offset = _ws(20) - B * N_INT * L_SITES * 20 * 4
    rc, err = _fwd(20, ws_bytes=srow_offset - 1)
    assert rc == TREX_E_ARG, rc
    assert b"workspace too small" in err
    rc, err = _fwd(20, ws_bytes=srow_offset, flags=2)
    assert rc == TREX_E_ARG, rc
    assert b"flags" in err


def test_bad_n_slots():
    rc, err = _fwd(4, n_slots=251)
    assert rc == TREX_E_ARG, rc
    assert b"bad n_slots" in err


def test_lds_too_deep_q4_generic(monkeypatch):
    monkeypatch.setenv("TREX_WIDE_SMALLQ", "0")  # the lane-per-site Q <= 4 kernel
    rc, err = _fwd(4, n_slots=250)
    assert rc == TREX_E_UNSUPPORTED, rc
    assert b"LDS stack too deep" in err


def test_lds_too_deep_q20_wide(monkeypatch):
    monkeypatch.setenv("TREX_STAGED", "0")  # tau = 0: not the site kernel; not staged: wide
    rc, err = _fwd(20, n_slots=250, tau=0.0)
    assert rc == TREX_E_UNSUPPORTED, rc
    assert b"LDS stack too deep" in err


def test_q129_unsupported():
    rc, err = _fwd(129)
    assert rc == TREX_E_UNSUPPORTED, rc
    assert b"not supported" in err


def test_ragged_phase0():
    rc, err = _ragged(phase=0)
    assert rc == TREX_E_ARG, rc
    assert b"phase" in err


def test_ragged_no_items():
    rc, err = _ragged(items=0)
    assert rc == TREX_E_ARG, rc
    assert b"bad shape" in err


@pytest.mark.parametrize("Q", [4, 20, 128])
def test_ragged_workspace_one_byte_short(Q):
    rc, err = _ragged(Q, ws_short=1)
    assert rc == TREX_E_ARG, rc
    assert b"workspace too small" in err
