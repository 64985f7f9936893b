"""Runs the host planner's entry points on one input and returns everything
they hand back (sizes, return codes, error texts, plan ints, info words) as
flat arrays: the generator of tests/golden/plan_cases.npz and
tests/test_plan_golden_cpu.py both go through here, so the fixture and the
test call the library the same way.  CPU only; numpy and ctypes."""

from __future__ import annotations

import contextlib
import os

import numpy as np

from trex_amd import lib

INTS_B = (0, 1)
INTS_N_ALL = (1, 2, 3, 4, 5, 65535, 65536)
INTS_FUNCS = ("trex_plan_ints", "trex_fused4_program_ints", "trex_nni_plan_ints",
              "trex_attach_plan_ints", "trex_ragged_plan_ints")


@contextlib.contextmanager
def defer_env(defer: bool):
    """TREX_DEFER unset (deferred cherry edges on) or "0" for the block."""
    old = os.environ.pop("TREX_DEFER", None)
    if not defer:
        os.environ["TREX_DEFER"] = "0"
    try:
        yield
    finally:
        os.environ.pop("TREX_DEFER", None)
        if old is not None:
            os.environ["TREX_DEFER"] = old


def _err(rc) -> np.ndarray:
    return np.array(lib().trex_last_error().decode() if rc else "")


def _buffer(n) -> np.ndarray:
    # a refused shape has no size: the build call is still made (for its
    # return code and error text) on a buffer it must not touch
    return np.zeros(n if n > 0 else 64, dtype=np.int32)


def _record(out, name, n, rc, buf, **extra):
    out[f"{name}_ints"] = np.int64(n)
    out[f"{name}_rc"] = np.int64(rc)
    out[f"{name}_err"] = _err(rc)
    if rc == 0:  # a failed build's buffer is not part of the contract
        out[name] = buf
        out.update({f"{name}_{k}": v for k, v in extra.items()})


def run_uniform(children, defer: bool) -> dict:
    """The main plan, the fused Q = 4 program of that plan, the NNI plan and
    the attach plan of one uniform batch (B, n_all, 2)."""
    L = lib()
    ch = np.ascontiguousarray(children, dtype=np.int32)
    B, n_all, _ = ch.shape
    out = {}
    with defer_env(defer):
        n = int(L.trex_plan_ints(B, n_all))
        plan = _buffer(n)
        info = np.zeros(4, dtype=np.int32)
        rc = L.trex_plan_build(ch.ctypes.data, B, n_all, plan.ctypes.data, info.ctypes.data)
        _record(out, "plan", n, rc, plan, info=info)
        n = int(L.trex_fused4_program_ints(B, n_all))
        out["fused4_ints"] = np.int64(n)
        if rc == 0:  # the program is built from a plan
            prog = _buffer(n)
            rc = L.trex_fused4_program_build(plan.ctypes.data, B, n_all, prog.ctypes.data)
            _record(out, "fused4", n, rc, prog)
        for name in ("nni", "attach"):
            n = int(getattr(L, f"trex_{name}_plan_ints")(B, n_all))
            buf = _buffer(n)
            rc = getattr(L, f"trex_{name}_plan_build")(ch.ctypes.data, B, n_all, buf.ctypes.data)
            _record(out, name, n, rc, buf)
    return out


def run_ragged(packed_children, n_all, sites, defer: bool) -> dict:
    """The ragged plan of trees of n_all[b] nodes and sites[b] sites; their
    child lists concatenated in packed_children (sum n_all, 2)."""
    L = lib()
    ch = np.ascontiguousarray(packed_children, dtype=np.int32)
    n_all = np.ascontiguousarray(n_all, dtype=np.int32)
    sites = np.ascontiguousarray(sites, dtype=np.int32)
    B = len(n_all)
    out = {}
    with defer_env(defer):
        n = int(L.trex_ragged_plan_ints(B, n_all.ctypes.data, sites.ctypes.data))
        plan = _buffer(n)
        info = np.zeros(8, dtype=np.int64)
        rc = L.trex_ragged_plan_build(ch.ctypes.data, n_all.ctypes.data, sites.ctypes.data, B,
                                      plan.ctypes.data, info.ctypes.data)
        _record(out, "plan", n, rc, plan, info=info)
    return out


def ints_table() -> np.ndarray:
    """int64 (len(INTS_FUNCS), len(INTS_B), len(INTS_N_ALL)): what every
    *_ints function returns; the ragged one on a batch of B trees of n_all
    nodes and 64 sites."""
    L = lib()
    out = np.zeros((len(INTS_FUNCS), len(INTS_B), len(INTS_N_ALL)), dtype=np.int64)
    for f, name in enumerate(INTS_FUNCS):
        for i, B in enumerate(INTS_B):
            for j, n_all in enumerate(INTS_N_ALL):
                if name == "trex_ragged_plan_ints":
                    na = np.full(max(B, 1), n_all, dtype=np.int32)
                    ls = np.full(max(B, 1), 64, dtype=np.int32)
                    out[f, i, j] = L.trex_ragged_plan_ints(B, na.ctypes.data, ls.ctypes.data)
                else:
                    out[f, i, j] = getattr(L, name)(B, n_all)
    return out
