"""State-set leaves: encoders from leaf codes and from alignment strings to
the int32 masks the scoring and search functions take in place of int8 codes
(DESIGN.md "State-set leaves").  Bit j of a cell = state j is allowed there.
Host numpy; nothing here touches the device.
"""

from __future__ import annotations

import numpy as np

_DNA_ORDER = "ACGT"
_DNA_SETS = {
    "A": "A", "C": "C", "G": "G", "T": "T", "U": "T",
    "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
    "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG",
    "N": "ACGT", "X": "ACGT", "?": "ACGT", "-": "ACGT",
}
_PROTEIN_ORDER = "ARNDCQEGHILKMFPSTWYV"
_PROTEIN_SETS = {**{a: a for a in _PROTEIN_ORDER}, "B": "DN", "Z": "EQ", "J": "IL",
                 **{a: _PROTEIN_ORDER for a in "X?-*"}}


def _table(order, sets):
    """256-entry byte -> mask table (-1: not a symbol), both letter cases."""
    t = np.full(256, -1, dtype=np.int64)
    for sym, states in sets.items():
        mask = sum(1 << order.index(s) for s in states)
        t[ord(sym.upper())] = t[ord(sym.lower())] = mask
    return t


ALPHABETS = {"dna": (4, _table(_DNA_ORDER, _DNA_SETS)),
             "protein": (20, _table(_PROTEIN_ORDER, _PROTEIN_SETS))}


def sets_from_codes(codes, n_states: int):
    """int8 leaf codes -> int32 masks of the same shape: code c in
    [0, n_states) gives ``1 << c``, anything else (the missing code -1) gives
    0, the mask whose row is all 1e5 as code -1's is."""
    if not 1 <= n_states <= 31:
        raise ValueError("n_states must be in [1, 31]")
    c = np.asarray(codes).astype(np.int64)
    ok = (c >= 0) & (c < n_states)
    return np.where(ok, np.left_shift(1, np.where(ok, c, 0)), 0).astype(np.int32)


def encode_alignment(seqs, alphabet: str = "dna"):
    """Equal-length strings -> int32 (n, L) masks; letters in either case.

    ``"dna"``: 4 states in the order A, C, G, T (U = T); R = AG, Y = CT,
    S = CG, W = AT, K = GT, M = AC, B = CGT, D = AGT, H = ACT, V = ACG;
    N, X, ?, - = all four.  ``"protein"``: 20 states in the order
    ARNDCQEGHILKMFPSTWYV; B = D|N, Z = E|Q, J = I|L; X, ?, -, * = all twenty.
    Any other character, and sequences of unequal length, raise ValueError.
    """
    if alphabet not in ALPHABETS:
        raise ValueError(f"alphabet must be one of {sorted(ALPHABETS)}, got {alphabet!r}")
    table = ALPHABETS[alphabet][1]
    seqs = list(seqs)
    if not seqs or not all(isinstance(s, str) for s in seqs):
        raise ValueError("seqs must be a non-empty list of strings")
    L = len(seqs[0])
    out = np.empty((len(seqs), L), dtype=np.int32)
    for i, s in enumerate(seqs):
        if len(s) != L:
            raise ValueError(f"sequence {i} has length {len(s)}, sequence 0 has {L}")
        b = np.frombuffer(s.encode("latin-1", errors="replace"), dtype=np.uint8)
        m = table[b]
        if not s.isascii():  # what latin-1 cannot hold was replaced by '?'
            m = np.where(np.array([ord(ch) > 255 for ch in s], dtype=bool), -1, m)
        bad = np.flatnonzero(m < 0)
        if bad.size:
            pos = int(bad[0])
            raise ValueError(f"character {s[pos]!r} at position {pos} of sequence {i} is not a "
                             f"{alphabet} symbol")
        out[i] = m
    return out
