"""Engine::manyPoint (reference src/Engine/Engine.h:341-389) for the S = 1/2 Heisenberg basis, as a chain of heis_obs_reference.acc_modified_state_
through the sectors of Heisenberg::hasNewPartsSplusOrMinus (Heisenberg.h:218-240): the first listed operator acts first, every step has factor 1, and the
bracket is 0 when the final sector differs from the first (:382-383).  Two conventions differ from the reference on purpose, both where it is ill-defined:
n and sz act in the sector the string has reached (getNeededBasis :397-400 hands them the original sector's basis), and S- throws when the CURRENT sector
is the all-down one (Heisenberg.h:233 tests the original szPlusConst).  Nothing here comes from the engine under test."""
import numpy as np

import heis_obs_reference as ref
from heis_obs_reference import DOWN, UP, Throws  # noqa: F401


def strings(L):
    """the 13 strings of the tests for a chain of L >= 7 sites; sites on both sides of the 12-bit cut exist from L = 14"""
    lo, hi, e = min(L, 12) - 1, min(12, L - 1), L - 1
    return [
        [("sz", 0, UP), ("sz", e, UP)],
        [("splus", 0, UP), ("sminus", hi, UP)],
        [("sminus", lo, UP), ("splus", hi, UP)],
        [("splus", 0, UP), ("sminus", 3, UP), ("splus", hi, UP), ("sminus", e, UP)],
        [("sz", 0, UP), ("sz", 3, UP), ("sz", lo, UP), ("sz", e, UP)],
        [("n", 0, UP), ("n", 3, DOWN), ("n", hi, UP)],
        [("sminus", 3, UP), ("sz", 3, UP), ("splus", 3, UP)],
        [("splus", 0, UP), ("splus", 0, UP)],  # dead
        [("splus", 0, UP), ("sz", hi, UP)],  # ends in another sector
        [("n", 0, UP), ("n", 0, DOWN)],  # dead
        [("splus", 0, UP), ("sminus", 3, UP), ("sz", hi, UP)],
        [("splus", 0, UP), ("sminus", 0, UP)] * 8,  # 16 operators
        [("sminus", e, UP), ("n", e, DOWN), ("sz", e, UP), ("splus", e, UP), ("sz", 1, UP)],
    ]


DEAD = (7, 9)  # indices of the strings that are identically zero
LEAVES = (8,)  # ... that end in another sector


def text(string):
    """the -M form of a string"""
    return ";".join("%s?%d?%d" % item for item in string)


def apply_string(string, L, m, src, factor=1.0):
    """(string src, final szPlusConst): accModifiedState_ step by step, the factor on the first step; raises Throws where S+ meets the all-up sector or
    S- the all-down one"""
    vec, cur = np.asarray(src), m
    assert len(vec) == ref.size(L, m)
    for k, (op, site, spin) in enumerate(string):
        if op not in ref.OPS:
            raise Throws("unknownOperator " + op)
        new = ref.new_sector(op, spin, L, cur)  # throws
        vec = ref.acc_modified_state_(np.zeros(ref.size(L, new), vec.dtype), op, L, cur, new, vec, site, spin, factor if k == 0 else 1.0)
        cur = new
    return vec, cur


def many_point(string, L, m, bra, ket):
    """conj(bra) . (string ket), 0 when the string ends in another sector"""
    vec, cur = apply_string(string, L, m, ket)
    return np.vdot(bra, vec) if cur == m else np.zeros((), vec.dtype)[()]


def action(string, L, m):
    """(destination -> +-(source + 1) or 0, final szPlusConst) by pushing a vector of source labels 1 .. N through the chain: every step maps one source
    to at most one destination with a value of -1, 0 or 1, so the labels survive exactly"""
    vec, cur = apply_string(string, L, m, np.arange(1, ref.size(L, m) + 1, dtype=np.float64))
    return np.rint(vec).astype(np.int64), cur
