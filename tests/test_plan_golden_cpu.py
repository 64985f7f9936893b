"""The host planner's output, pinned bit for bit (tests/golden/plan_cases.npz,
written by tests/golden/make_golden.py): every plan int, info word, size,
return code and error text of trex_plan_build, trex_fused4_program_build,
trex_nni_plan_build, trex_attach_plan_build and trex_ragged_plan_build on a
corpus of ordinary, quirky and refused child lists, with TREX_DEFER unset and
"0", and what every *_ints function returns on edge shapes.  The buffer of a
refused build is not compared.  No kernel is launched here."""

from __future__ import annotations

import os

import numpy as np
import pytest

from _plan_golden import ints_table, run_ragged, run_uniform

GOLDEN = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                   "plan_cases.npz")))
MODES = ("defer", "nodefer")


def _names(prefix):
    return sorted({k.split("/")[1] for k in GOLDEN if k.startswith(prefix + "/")})


def _assert_same(got, prefix):
    want = {k[len(prefix):]: v for k, v in GOLDEN.items() if k.startswith(prefix)}
    assert want and sorted(got) == sorted(want)
    for key, val in want.items():
        g = np.asarray(got[key])
        assert g.dtype == val.dtype and g.shape == val.shape, key
        assert np.array_equal(g, val), f"{prefix}{key} differs"


def test_corpus_is_complete():
    """The cases the fixture must hold, and that it pins refusals too."""
    u = _names("u")
    for name in ["random3", "random4", "random8", "random16", "random40", "random64",
                 "balanced64", "caterpillar33", "fwdref", "dag", "cycle", "unreached", "n_all3",
                 "n_all4", "malformed"]:
        assert name in u
    assert len(_names("r")) >= 2 + 2
    assert {1, 64, 65} <= set(GOLDEN["r/a/sites"].tolist()) | set(GOLDEN["r/b/sites"].tolist())
    rc = {n: int(GOLDEN[f"u/{n}/defer/plan_rc"]) for n in u}
    assert rc["malformed"] == -2 and all(v == 0 for n, v in rc.items() if n != "malformed")
    texts = {str(GOLDEN[k]) for k in GOLDEN if k.endswith("_err")}
    for part in ["1e5-sentinel child", "two parents", "does not reach", "bad arguments",
                 "has no NNI neighbours", "is not supported (3 or more", "invalid child list"]:
        assert any(part in t for t in texts), part


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", _names("u"))
def test_uniform_plans_match_golden(name, mode):
    got = run_uniform(GOLDEN[f"u/{name}/children"], mode == "defer")
    _assert_same(got, f"u/{name}/{mode}/")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", _names("r"))
def test_ragged_plans_match_golden(name, mode):
    got = run_ragged(GOLDEN[f"r/{name}/children"], GOLDEN[f"r/{name}/n_all"],
                     GOLDEN[f"r/{name}/sites"], mode == "defer")
    _assert_same(got, f"r/{name}/{mode}/")


def test_ints_functions_match_golden():
    assert np.array_equal(ints_table(), GOLDEN["ints"])
