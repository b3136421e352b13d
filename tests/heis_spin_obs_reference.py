"""Literal restatement of the one-site observables of the spin-S Heisenberg digit basis (the project's own definition: the reference throws for spins
above 1/2, BasisHeisenberg.h:130,263, Heisenberg.h:223).  The basis is BasisHeisenberg.h:24-47: L digits of `bits` bits each, site p at bit offset
p * bits, digit d = m + S in [0, twiceS], the words whose digits add up to szPlusConst, ascending as integers.  With m = d - S of the SOURCE state
    splus   digit d -> d + 1, value sqrt(S(S+1) - m(m+1)), nothing leaves d = twiceS
    sminus  digit d -> d - 1, value sqrt(S(S+1) - m(m-1)), nothing leaves d = 0
    sz      index kept, value m; a value of 0 leaves the destination untouched
The words are listed by recursion from the most significant digit and indices are found in a dictionary: nothing here knows about runs, ranks or
counting tables, and nothing comes from the engine under test.  two_point, modified_state and spectral_types follow Engine::twoPoint /
getModifiedState / spectralFunction (src/Engine/Engine.h:266-338, :494-533, :134-206) with these operators."""
import math
from functools import lru_cache

import numpy as np

OPS = ("sz", "splus", "sminus")
ALL_OPS = ("c", "cdagger", "n", "sz", "splus", "sminus")
NEEDS_NEW_BASIS = ("splus", "sminus")
TRANSPOSE_CONJUGATE = {"splus": "sminus", "sminus": "splus", "sz": "sz"}


class Refused(RuntimeError):
    """the definition refuses here (LPP_ERR_INVALID in the engine)"""


def bits_of(L, twiceS):
    """the digit width of the assembler (BasisHeisenberg.h:28-46): 1 + floor(log2(twiceS + 1)), one less for odd twiceS; odd twiceS only when
    twiceS + 1 is a power of two; bits * L <= 62"""
    if L < 1 or twiceS < 1:
        raise Refused("bad sites / twiceS")
    bits = 1 + int(math.floor(math.log2(twiceS + 1)))
    if twiceS & 1:
        bits -= 1
        if (1 << bits) - 1 < twiceS:
            raise Refused("odd twiceS with twiceS + 1 not a power of two")
    if bits * L > 62:
        raise Refused("bits * L > 62")
    return bits


@lru_cache(maxsize=64)
def basis(L, twiceS, m):
    """(words ascending, {word: index}): by recursion from the most significant digit, smaller digits first"""
    bits = bits_of(L, twiceS)
    if m < 0 or m > L * twiceS:
        raise Refused("empty Hilbert space")
    words = []

    def rec(site, word, left):
        if site < 0:
            if left == 0:
                words.append(word)
            return
        for d in range(min(twiceS, left) + 1):
            if left - d <= site * twiceS:  # the sites below can still hold what remains
                rec(site - 1, word | (d << (site * bits)), left - d)

    rec(L - 1, 0, m)
    assert words == sorted(words)
    return words, {w: i for i, w in enumerate(words)}


def size(L, twiceS, m):
    return len(basis(L, twiceS, m)[0])


def value(op, twiceS, d):
    """the operator's value on a source state whose digit at the site is d"""
    spin = twiceS * 0.5
    m = d - spin
    if op == "splus":
        return math.sqrt(spin * (spin + 1.0) - m * (m + 1.0))
    if op == "sminus":
        return math.sqrt(spin * (spin + 1.0) - m * (m - 1.0))
    return m


def has_new_parts(op, L, twiceS, m, spin=0):
    """the new szPlusConst of splus / sminus, None for sz; n, c, cdagger, S+ on the top sector, S- on szPlusConst = 0 and a bad spin are refused"""
    bits_of(L, twiceS)
    if spin not in (0, 1):
        raise Refused("bad spin")
    if m < 0 or m > L * twiceS:
        raise Refused("bad sector")
    if op == "sz":
        return None
    if op == "splus":
        if m + 1 > L * twiceS:
            raise Refused("S+ on the top sector")
        return m + 1
    if op == "sminus":
        if m == 0:
            raise Refused("S- on szPlusConst = 0")
        return m - 1
    raise Refused("unsupported operator " + op)


def new_sector(op, L, twiceS, m):
    new = has_new_parts(op, L, twiceS, m)
    return m if new is None else new


@lru_cache(maxsize=512)
def action(op, L, twiceS, m, site):
    """for every ket of the source sector: (bra index or -1, value)"""
    if op not in OPS:
        raise Refused("unsupported operator " + op)
    bits = bits_of(L, twiceS)
    new_m = new_sector(op, L, twiceS, m)
    kets = basis(L, twiceS, m)[0]
    find = basis(L, twiceS, new_m)[1]
    index = np.full(len(kets), -1, np.int64)
    val = np.zeros(len(kets))
    for k, w in enumerate(kets):
        d = (w >> (site * bits)) & ((1 << bits) - 1)
        if op == "splus":
            if d == twiceS:
                continue
            bra = w + (1 << (site * bits))
        elif op == "sminus":
            if d == 0:
                continue
            bra = w - (1 << (site * bits))
        else:
            bra = w
        index[k] = find[bra]
        val[k] = value(op, twiceS, d)
    return index, val


def apply(z, op, L, twiceS, m, src, site, factor=1.0):
    """z[bra] += factor * value * src[ket]; a value of 0 adds 0"""
    index, val = action(op, L, twiceS, m, site)
    ok = index >= 0
    np.add.at(z, index[ok], (factor * val[ok]) * src[ok])
    return z


def touched(op, L, twiceS, m, site):
    """the destinations an application changes: a bra index with a value other than 0"""
    index, val = action(op, L, twiceS, m, site)
    t = np.zeros(size(L, twiceS, new_sector(op, L, twiceS, m)), bool)
    t[index[(index >= 0) & (val != 0)]] = True
    return t


def two_point(op, L, twiceS, m, bra, ket):
    """(result, trace) with result[i][j] = <A_j bra | A_i ket>"""
    n = size(L, twiceS, new_sector(op, L, twiceS, m))
    m2 = [apply(np.zeros(n, ket.dtype), op, L, twiceS, m, bra, j) for j in range(L)]
    result = np.zeros((L, L), ket.dtype)
    total = 0.0
    for i in range(L):
        m1 = apply(np.zeros(n, ket.dtype), op, L, twiceS, m, ket, i)
        for j in range(L):
            result[i, j] = np.vdot(m2[j], m1)
        total = total + result[i, i]
    return result, total


def modified_state(op, L, twiceS, m, gs, typ, isite, jsite):
    """A_i |gs> + isign A_j |gs>; a diagonal pair is accumulated twice"""
    z = np.zeros(size(L, twiceS, new_sector(op, L, twiceS, m)), gs.dtype)
    apply(z, op, L, twiceS, m, gs, isite, 1.0)
    return apply(z, op, L, twiceS, m, gs, jsite, -1.0 if typ > 1 else 1.0)


def spectral_types(op, L, twiceS, m, gs, isite, jsite):
    """the loop of Engine::spectralFunction (:160-205): [(type, operator of the type, new szPlusConst, modified vector, weight * s2, -s)]; the
    operators are bosonic; a type whose operator is refused (S+ on the top sector, S- on szPlusConst = 0) raises, as the engine does"""
    out = []
    op2 = TRANSPOSE_CONJUGATE[op]
    diagonal = isite == jsite
    for typ in range(4):
        if diagonal and typ > 1:
            continue
        o = op if (typ & 1) else op2
        new_m = new_sector(o, L, twiceS, m)
        modif = modified_state(o, L, twiceS, m, gs, typ, isite, jsite)
        weight = np.vdot(modif, modif).real
        s = -1 if (typ & 1) else 1
        s2 = (-1.0 if typ > 1 else 1.0) * s * (1.0 if diagonal else 0.5)
        out.append((typ, o, new_m, modif, weight * s2, -s))
    return out


def plan_action(plan, n_src):
    """the engine's expanded plan (lanczosplusplus_amd.operator_plan_heis_spin: action[dst] = src + 1 or 0, coef[dst]) in the form of action(): for
    every ket the bra index or -1 and the coefficient.  A source named twice would be an error of the plan."""
    a = plan["action"]
    assert a.min() >= 0
    dst = np.nonzero(a)[0]
    src = a[dst] - 1
    assert len(np.unique(src)) == len(src) and (len(src) == 0 or src.max() < n_src)
    index = np.full(n_src, -1, np.int64)
    coef = np.zeros(n_src)
    index[src] = dst
    coef[src] = plan["coef"][dst]
    assert not np.any(plan["coef"][a == 0])
    return index, coef
