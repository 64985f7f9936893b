"""State-set leaves without a GPU: the encoders, compress_sites on masks, the
presence of the entry points, and their argument checks (every call below is
rejected before any launch, so host numpy buffers stand in for device
pointers as in tests/test_args_cpu.py)."""

from __future__ import annotations

import numpy as np
import pytest

from trex_amd import compress_sites, encode_alignment, sets_from_codes
from trex_amd._lib import TREX_E_ARG, TREX_E_UNSUPPORTED, has_leaf_sets, lib

DNA = {"A": 1, "C": 2, "G": 4, "T": 8, "U": 8, "R": 5, "Y": 10, "S": 6, "W": 9, "K": 12, "M": 3,
       "B": 14, "D": 13, "H": 11, "V": 7, "N": 15, "X": 15, "?": 15, "-": 15}
PROTEIN_ORDER = "ARNDCQEGHILKMFPSTWYV"


def test_dna_table_every_symbol_both_cases():
    syms = "".join(DNA)
    got = encode_alignment([syms, syms.lower()], "dna")
    assert got.dtype == np.int32 and got.shape == (2, len(syms))
    want = np.array([DNA[s] for s in syms], dtype=np.int32)
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[1], want)
    np.testing.assert_array_equal(encode_alignment([syms]), got[:1])  # "dna" is the default


def test_protein_table_every_symbol_both_cases():
    bit = {a: 1 << i for i, a in enumerate(PROTEIN_ORDER)}
    table = dict(bit)
    table.update(B=bit["D"] | bit["N"], Z=bit["E"] | bit["Q"], J=bit["I"] | bit["L"])
    for s in "X?-*":
        table[s] = (1 << 20) - 1
    syms = "".join(table)
    got = encode_alignment([syms, syms.lower()], "protein")
    want = np.array([table[s] for s in syms], dtype=np.int32)
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[1], want)
    assert len(table) == 27  # 20 + B Z J + X ? - *


@pytest.mark.parametrize("alphabet,bad", [("dna", "Z"), ("dna", "*"), ("dna", "E"),
                                          ("protein", "O"), ("protein", "U"), ("dna", " "),
                                          ("dna", "é"), ("dna", "中")])
def test_bad_character_names_itself_its_sequence_and_position(alphabet, bad):
    with pytest.raises(ValueError) as e:
        encode_alignment(["ACGA", "AC" + bad + "A"], alphabet)
    msg = str(e.value)
    assert repr(bad) in msg and "position 2" in msg and "sequence 1" in msg, msg


def test_unequal_lengths_and_unknown_alphabet():
    with pytest.raises(ValueError, match="length"):
        encode_alignment(["ACGT", "ACG"])
    with pytest.raises(ValueError, match="alphabet"):
        encode_alignment(["ACGT"], "rna")


def test_sets_from_codes():
    codes = np.array([[0, 1, 2, 3], [-1, 4, 127, -128]], dtype=np.int8)
    got = sets_from_codes(codes, 4)
    assert got.dtype == np.int32 and got.shape == codes.shape
    np.testing.assert_array_equal(got, [[1, 2, 4, 8], [0, 0, 0, 0]])
    np.testing.assert_array_equal(sets_from_codes(np.arange(20, dtype=np.int8), 20),
                                  1 << np.arange(20))


def test_compress_sites_on_masks_and_unchanged_on_codes():
    rng = np.random.default_rng(0)
    # masks that differ only above the low byte are different symbols
    masks = rng.integers(0, 3, size=(5, 40)).astype(np.int32) * 0x101 + 1
    masks[:, 7] = masks[:, 3]
    pat, counts, index = compress_sites(masks)
    assert pat.dtype == np.int32 and counts.dtype == np.float32 and index.dtype == np.int64
    np.testing.assert_array_equal(pat[:, index], masks)
    np.testing.assert_array_equal(counts, np.bincount(index, minlength=pat.shape[1]))
    assert len({tuple(c) for c in pat.T}) == pat.shape[1] < 40
    first = [int(np.flatnonzero(index == p)[0]) for p in range(pat.shape[1])]
    assert first == sorted(first)  # order of first occurrence
    lo = np.array([[1, 1], [2, 2]], dtype=np.int32)
    hi = lo.copy()
    hi[0, 1] |= 1 << 16
    assert compress_sites(lo)[0].shape[1] == 1 and compress_sites(hi)[0].shape[1] == 2
    # int8 codes: as before
    codes = rng.integers(-1, 4, size=(5, 40)).astype(np.int8)
    pat8, counts8, index8 = compress_sites(codes)
    assert pat8.dtype == np.int8
    np.testing.assert_array_equal(pat8[:, index8], codes)
    pat64 = compress_sites(codes.astype(np.int64))[0]
    assert pat64.dtype == np.int8
    np.testing.assert_array_equal(pat64, pat8)


def test_entry_points_present_and_version_unchanged():
    assert has_leaf_sets()
    assert lib().trex_version() == 10
    assert lib().trex_sets_fwd_workspace_bytes(3, 65, 9, 4) == 3 * 2 * 8 + 256
    assert lib().trex_sets_fwd_workspace_bytes(3, 65, 9, 21) == 0


# ---- C ABI argument checks -------------------------------------------------
B, L, N_ALL = 1, 64, 7


def _call(name, Q=4, tau=0.0, flags=0, sub_sets=True, sub_rows=False, short=False):
    """(return code, error text) of one entry point on host stand-ins.  Only
    ever called with arguments the library must refuse before it launches."""
    Lb = lib()
    b = np.zeros(1 << 16, np.uint8)
    p = b.ctypes.data
    size_of = {"fwd": Lb.trex_sets_fwd_workspace_bytes, "nni": Lb.trex_nni_workspace_bytes,
               "attach": Lb.trex_attach_workspace_bytes}
    nb = 0
    if name in size_of:
        nb = int(size_of[name](B, L, N_ALL, min(Q, 20)))
        assert nb > 0
    w = np.zeros(nb + 1, np.uint8).ctypes.data
    if short:
        nb -= 1
    if name == "fwd":
        rc = Lb.trex_sankoff_sets_fwd(p, p, p, B, L, N_ALL, Q, tau, flags, p, None, p, w, nb, None)
    elif name == "outside":
        rc = Lb.trex_sankoff_sets_outside(p, p, p, B, L, N_ALL, Q, tau, p, p, None)
    elif name == "nni":
        rc = Lb.trex_sankoff_sets_nni_w(p, p, p, B, L, N_ALL, Q, tau, p, p, None, p, w, nb, None)
    else:
        rc = Lb.trex_sankoff_sets_attach_w(p, p, p, B, L, N_ALL, Q, tau, p, p,
                                           p if sub_sets else None, p if sub_rows else None,
                                           None, p, w, nb, None)
    return rc, Lb.trex_last_error()


ALL4 = ("fwd", "outside", "nni", "attach")


@pytest.mark.parametrize("name", ALL4)
@pytest.mark.parametrize("tau", [float("nan"), float("inf"), -float("inf"), -1.0, -1e-30])
def test_bad_tau_is_rejected(name, tau):
    rc, err = _call(name, tau=tau)
    assert rc == TREX_E_ARG and b"tau" in err, (rc, err)


@pytest.mark.parametrize("flags", [2, 3, 4, 0x80000000])
def test_unknown_flags_are_rejected_by_the_forward(flags):
    rc, err = _call("fwd", tau=0.5, flags=flags)
    assert rc == TREX_E_ARG and b"flags" in err, (rc, err)


@pytest.mark.parametrize("sub_sets,sub_rows", [(True, True), (False, False)])
def test_both_or_neither_subtree_argument(sub_sets, sub_rows):
    rc, err = _call("attach", sub_sets=sub_sets, sub_rows=sub_rows)
    assert rc == TREX_E_ARG and b"sub_sets" in err and b"sub_rows" in err, (rc, err)


@pytest.mark.parametrize("name", ALL4)
def test_q21_is_unsupported(name):
    rc, err = _call(name, Q=21)
    assert rc == TREX_E_UNSUPPORTED, (rc, err)


@pytest.mark.parametrize("name", ["fwd", "nni", "attach"])
def test_too_small_workspace(name):
    rc, err = _call(name, short=True)
    assert rc == TREX_E_ARG and b"workspace" in err, (rc, err)
