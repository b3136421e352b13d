"""Engine::manyPoint (reference src/Engine/Engine.h:341-389) for the one-orbital t-J basis, as a chain of tj_obs_reference.acc_modified_state_ through
the sectors of TjMultiOrb::hasNewParts (tj_obs_reference.new_sector) on the sorted word list: the first listed operator acts first, every step has
factor 1, a step without a sector ends the chain ("no sector", the value is 0), and the bracket is 0 when the final sector differs from the first
(:382-383).  One convention differs from the reference on purpose, where it is ill-defined: n and sz act in the sector the string has reached
(getNeededBasis :397-400 hands them the original sector's basis).  Nothing here comes from the engine under test."""
import numpy as np

import tj_obs_reference as ref
from tj_obs_reference import DOWN, UP  # noqa: F401


def strings(L):
    """the 15 strings of the tests for L >= 6 sites"""
    e, h = L - 1, L // 2
    return [
        [("n", 0, UP), ("n", e, DOWN)],
        [("sz", 1, UP), ("sz", 1, UP)],
        [("c", 0, UP), ("cdagger", h, UP)],
        [("c", e, DOWN), ("cdagger", 1, DOWN)],
        [("c", 0, UP), ("c", 1, DOWN), ("cdagger", e, DOWN), ("cdagger", h, UP)],
        [("splus", 0, UP), ("sminus", e, UP)],
        [("sminus", h, UP), ("splus", 1, UP)],
        [("sminus", 2, UP), ("n", 2, DOWN), ("splus", 2, UP)],
        [("c", 3, UP), ("cdagger", 3, DOWN), ("sz", 3, DOWN), ("splus", 3, UP), ("n", 3, UP), ("c", 3, UP), ("cdagger", 3, UP)],
        [("c", 0, UP), ("c", 0, UP)],  # dead, or no sector when nup = 1
        [("n", 0, UP), ("n", 0, DOWN)],  # dead
        [("c", 0, UP), ("n", h, DOWN)],  # ends elsewhere
        [("c", 2, DOWN), ("cdagger", 2, UP)],  # ends elsewhere
        [("c", 1, UP), ("cdagger", 1, UP)] * 8,  # 16 operators
        [("splus", 1, UP), ("sminus", h, UP), ("c", 0, UP), ("cdagger", 0, UP)],
    ]


def text(string):
    """the -M form of a string"""
    return ";".join("%s?%d?%d" % item for item in string)


def apply_string(string, L, parts, src, factor=1.0):
    """(string src, final parts) by accModifiedState_ step by step, the factor on the first step; (None, None) where a step leads to no sector"""
    vec, cur = np.asarray(src), tuple(parts)
    assert len(vec) == ref.size(L, *cur)
    for k, (op, site, spin) in enumerate(string):
        new = ref.new_sector(op, spin, L, *cur)
        if new is None:
            return None, None
        vec = ref.acc_modified_state_(np.zeros(ref.size(L, *new), vec.dtype), op, L, cur, tuple(new), vec, site, spin, factor if k == 0 else 1.0)
        cur = tuple(new)
    return vec, cur


def many_point(string, L, parts, bra, ket):
    """conj(bra) . (string ket); 0 when the string leads to no sector or ends in another one"""
    vec, cur = apply_string(string, L, parts, ket)
    zero = np.zeros((), np.result_type(np.asarray(bra).dtype, np.asarray(ket).dtype))[()]
    return np.vdot(bra, vec) if vec is not None and cur == tuple(parts) else zero


def action(string, L, parts):
    """(destination -> +-(source + 1) or 0, final parts) by pushing a vector of source labels 1 .. N through the chain: every step maps one source to
    at most one destination with a value of -1, 0 or 1, so the labels survive exactly; (None, None) where a step leads to no sector"""
    vec, cur = apply_string(string, L, parts, np.arange(1, ref.size(L, *parts) + 1, dtype=np.float64))
    return (None, None) if vec is None else (np.rint(vec).astype(np.int64), cur)
