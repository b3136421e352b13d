"""Literal numpy restatement of the reference's observable code for BasisHubbardLanczos, on top of oracle.hubbard_basis_words:
getBraIndex / doSignGf / doSignSpSm (src/Models/HubbardOneOrbital/BasisHubbardLanczos.h:106-246), BasisOneSpin::getBra (BasisOneSpin.h:121-149),
hasNewParts (HubbardOneOrbital.h:87-109, :212-253), Engine::accModifiedState_ / accModifiedState / getModifiedState / calcSpectral / twoPoint
(src/Engine/Engine.h).  Vectorised over the kets of a sector; nothing here comes from the engine under test."""
from functools import lru_cache
from math import comb

import numpy as np

import oracle

UP, DOWN = 0, 1
OPS = ("c", "cdagger", "n", "sz", "splus", "sminus")
FERMIONIC = ("c", "cdagger")
NEEDS_NEW_BASIS = ("c", "cdagger", "splus", "sminus")
TRANSPOSE_CONJUGATE = {"c": "cdagger", "cdagger": "c", "splus": "sminus", "sminus": "splus", "n": "n", "sz": "sz"}


def popcount(w):
    w = np.asarray(w, np.uint64)
    n = np.zeros(w.shape, np.int64)
    for b in range(int(w.max()).bit_length() if w.size else 0):
        n += ((w >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
    return n


def has_new_parts(op, spin, L, nup, ndown):
    """HubbardOneOrbital::hasNewParts: the new parts, or None for `false`; raises for an unsupported operator"""
    if op in ("c", "cdagger"):
        p1, p2 = nup, ndown
        c = -1 if op == "c" else 1
        if spin == UP:
            p1 += c
        else:
            p2 += c
        if p1 < 0 or p2 < 0:
            return None
        if p1 > L or p2 > L:
            return None
        if p1 == 0 and p2 == 0:
            return None
        return p1, p2
    if op in ("splus", "sminus"):
        c = 1 if op == "splus" else -1
        p1, p2 = nup + c, ndown - c
        if p1 < 0 or p2 < 0:
            return None
        if p1 > L or p2 > L:
            return None
        return p1, p2
    if op == "sz":
        return None
    raise RuntimeError("hasNewParts: unsupported operator " + op)


def new_sector(op, spin, L, nup, ndown):
    """the sector an operator application writes into (needsNewBasis, LabeledOperator.h:83-90), or None"""
    if op in NEEDS_NEW_BASIS:
        return has_new_parts(op, spin, L, nup, ndown)
    return nup, ndown


def _species_basis(L, n):
    return oracle.onespin_basis(L, n) if comb(L, n) > 0 else np.zeros(0, np.uint64)


def _perfect_index(basis, words):
    """BasisOneSpin::perfectIndex: the position of a word in the ascending basis of its popcount"""
    idx = np.searchsorted(basis, words)
    idx = np.minimum(idx, max(len(basis) - 1, 0))
    assert len(basis) > 0 and np.array_equal(basis[idx], words)
    return idx.astype(np.int64)


def _get_bra(ket, op, site):
    """BasisOneSpin::getBra: (ok, bra)"""
    bit = np.uint64(1 << site)
    si = (ket & bit) > 0
    if op == "c":
        return si, ket ^ bit
    if op == "cdagger":
        return ~si, ket ^ bit
    if op == "n":
        return si, ket.copy()
    raise RuntimeError("Unknown operator " + op)


def get_bra_index(L, new_parts, ket1, ket2, op, site, spin):
    """BasisHubbardLanczos::getBraIndex over arrays of kets: (index or -1, value)"""
    b1, b2 = _species_basis(L, new_parts[0]), _species_basis(L, new_parts[1])
    n = len(ket1)
    index = np.full(n, -1, np.int64)
    value = np.ones(n, np.float64)

    def perfect(ok, w1, w2):
        if np.any(ok):
            index[ok] = _perfect_index(b1, w1[ok]) + _perfect_index(b2, w2[ok]) * len(b1)

    if op in ("splus", "sminus"):  # getBraIndexSplusSminus
        sp = UP if op == "splus" else DOWN
        k_sp, k_other = (ket1, ket2) if sp == UP else (ket2, ket1)
        ok1, brar1 = _get_bra(k_sp, "cdagger", site)
        ok2, brar2 = _get_bra(k_other, "c", site)
        ok = ok1 & ok2
        if sp == UP:
            perfect(ok, brar1, brar2)
        else:
            perfect(ok, brar2, brar1)
        return index, value
    if op == "sz":  # getBraIndexSz
        o1, _ = _get_bra(ket1, "n", site)
        o2, _ = _get_bra(ket2, "n", site)
        ok = o1 ^ o2
        perfect(ok, ket1, ket2)
        value = np.where(o1, 1.0, -1.0)
        return index, value
    if spin == UP:
        ok, bra = _get_bra(ket1, op, site)
        perfect(ok, bra, ket2)
    else:
        ok, bra = _get_bra(ket2, op, site)
        perfect(ok, ket1, bra)
    return index, value


def do_sign_gf(a, b, ind, sector):
    """BasisHubbardLanczos::doSignGf, line by line"""
    one = np.ones(len(a), np.int64)
    if sector == UP:
        if ind == 0:
            return one
        mask = a & np.uint64(((1 << 1) - 1) ^ ((1 << ind) - 1))
        s = np.where(popcount(mask) & 1, -1, 1)
        return np.where((a & np.uint64(1)) > 0, -s, s)
    s = np.where(popcount(a) & 1, -1, 1)  # parity of up
    if ind == 0:
        return s
    mask = b & np.uint64(((1 << 1) - 1) ^ ((1 << ind) - 1))
    s = np.where(popcount(mask) & 1, -1, 1)  # overwrites the up parity
    return np.where((b & np.uint64(1)) > 0, -s, s)


def _pg_do_sign(a, i):
    """ProgramGlobals::doSign"""
    return np.where(popcount(a & np.uint64((1 << i) - 1)) & 1, -1, 1)


def do_sign_spsm(a, b, ind):
    return _pg_do_sign(a, ind) * _pg_do_sign(b, ind)


@lru_cache(maxsize=4)
def _words(L, nup, ndown):
    return oracle.hubbard_basis_words(L, nup, ndown)


@lru_cache(maxsize=64)
def action(op, L, old_parts, new_parts, site, spin):
    """what accModifiedState_ does for every ket of the source sector: (bra index or -1, mysign * value)"""
    ket1, ket2 = _words(L, old_parts[0], old_parts[1])
    index, value = get_bra_index(L, new_parts, ket1, ket2, op, site, spin)
    mysign = do_sign_gf(ket1, ket2, site, spin).astype(np.float64) if op in FERMIONIC else np.ones(len(ket1))
    if op in ("splus", "sminus"):
        mysign = mysign * do_sign_spsm(ket1, ket2, site)
    return index, mysign * value


def acc_modified_state_(z, op, L, old_parts, new_parts, src, site, spin, factor):
    """Engine::accModifiedState_: z[temp] += factor*mysign*value*srcVector[ispace]"""
    index, sv = action(op, L, old_parts, new_parts, site, spin)
    m = index >= 0
    np.add.at(z, index[m], (factor * sv[m]) * src[m])
    return z


def acc_modified_state(z, op, L, old_parts, new_parts, src, site, spin, isign):
    """Engine::accModifiedState (the operator twoPoint applies)"""
    if op == "n":
        return acc_modified_state_(z, "n", L, old_parts, new_parts, src, site, spin, isign)
    if op == "sz":
        acc_modified_state_(z, "n", L, old_parts, new_parts, src, site, UP, isign * 0.5)
        return acc_modified_state_(z, "n", L, old_parts, new_parts, src, site, DOWN, -isign * 0.5)
    return acc_modified_state_(z, op, L, old_parts, new_parts, src, site, spin, isign)


def two_point(op, L, parts, bra, ket, spins):
    """Engine::twoPoint: (result, MatrixDiagonal); the matrix stays at -100 where the sector does not exist"""
    result = np.full((L, L), -100.0, dtype=ket.dtype)
    new_parts = parts
    if op in NEEDS_NEW_BASIS:
        assert spins[0] == spins[1]
        new_parts = has_new_parts(op, spins[0], L, parts[0], parts[1])
        if new_parts is None:
            return result, 0.0
    n = comb(L, new_parts[0]) * comb(L, new_parts[1])
    m2 = [acc_modified_state(np.zeros(n, ket.dtype), op, L, parts, new_parts, bra, j, spins[1], 1.0) for j in range(L)]
    total = 0.0
    for i in range(L):
        m1 = acc_modified_state(np.zeros(n, ket.dtype), op, L, parts, new_parts, ket, i, spins[0], 1.0)
        for j in range(L):
            result[i, j] = np.vdot(m2[j], m1)
            if i == j:
                total = total + result[i, i]
    return result, total


def modified_state(op, L, parts, new_parts, gs, typ, isite, jsite, spin):
    """Engine::getModifiedState (not the Tj1Orb branch): for isite == jsite the state is accumulated twice"""
    n = comb(L, new_parts[0]) * comb(L, new_parts[1])
    z = np.zeros(n, gs.dtype)
    acc_modified_state_(z, op, L, parts, new_parts, gs, isite, spin, 1.0)
    isign = -1.0 if typ > 1 else 1.0
    acc_modified_state_(z, op, L, parts, new_parts, gs, jsite, spin, isign)
    return z


def spectral_types(op, L, parts, gs, isite, jsite, spin):
    """the loop of Engine::spectralFunction: [(type, operator of the type, new parts, modified vector, weight*s2, -s)]"""
    out = []
    op2 = TRANSPOSE_CONJUGATE[op]
    diagonal = isite == jsite
    for typ in range(4):
        if diagonal and typ > 1:
            continue
        o = op if (typ & 1) else op2
        new_parts = parts
        if o in NEEDS_NEW_BASIS:
            new_parts = has_new_parts(o, spin, L, parts[0], parts[1])
            if new_parts is None:
                continue
        modif = modified_state(o, L, parts, new_parts, gs, typ, isite, jsite, spin)
        weight = np.vdot(modif, modif).real
        s = -1 if (typ & 1) else 1  # calcSpectral
        s2 = -1.0 if typ > 1 else 1.0
        if o not in FERMIONIC:
            s2 *= s
        s2 *= 1.0 if diagonal else 0.5
        out.append((typ, o, new_parts, modif, weight * s2, -s))
    return out


def jordan_wigner(op, L, parts, new_parts, site, spin):
    """c / cdagger of one spin-orbital as the textbook Jordan-Wigner operator, modes ordered (up, site 0..L-1), (down, site 0..L-1):
    for every ket of `parts` the bra index in `new_parts` (or -1) and the sign (-1)^(occupied modes before the one acted on)."""
    ket1, ket2 = oracle.hubbard_basis_words(L, parts[0], parts[1])
    b1, b2 = _species_basis(L, new_parts[0]), _species_basis(L, new_parts[1])
    bit = np.uint64(1 << site)
    below = np.uint64((1 << site) - 1)
    word = ket1 if spin == UP else ket2
    occ = (word & bit) > 0
    ok = occ if op == "c" else ~occ
    before = popcount(word & below) + (popcount(ket1) if spin == DOWN else 0)
    sign = np.where(before & 1, -1.0, 1.0)
    index = np.full(len(ket1), -1, np.int64)
    w1 = np.where(ok, ket1 ^ bit, ket1) if spin == UP else ket1
    w2 = np.where(ok, ket2 ^ bit, ket2) if spin == DOWN else ket2
    if np.any(ok):
        index[ok] = _perfect_index(b1, w1[ok]) + _perfect_index(b2, w2[ok]) * len(b1)
    return index, sign


def tables_action(plan, op, L, parts):
    """the engine's per-species tables (lanczosplusplus_amd.operator_plan) turned into the same form as action(): for every ket of `parts` the bra
    index or -1 and the coefficient"""
    tu, td = plan["table_up"].astype(np.int64), plan["table_down"].astype(np.int64)
    nu_src = comb(L, parts[0])
    n_src = nu_src * comb(L, parts[1])
    index = np.full(n_src, -1, np.int64)
    coef = np.zeros(n_src)
    du, dd = np.meshgrid(np.arange(len(tu)), np.arange(len(td)))  # dd major
    du, dd = du.ravel(), dd.ravel()
    dst = du + dd * len(tu)
    if op == "sz":
        v = (tu[du] != 0).astype(np.int64) - (td[dd] != 0).astype(np.int64)
        m = v != 0
        index[dst[m]] = dst[m]
        coef[dst[m]] = v[m]
        return index, coef
    m = (tu[du] != 0) & (td[dd] != 0)
    src = (np.abs(tu[du][m]) - 1) + (np.abs(td[dd][m]) - 1) * nu_src
    assert len(np.unique(src)) == len(src)
    index[src] = dst[m]
    coef[src] = np.sign(tu[du][m]) * np.sign(td[dd][m])
    return index, coef
