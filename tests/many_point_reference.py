"""Oracles for products of one-site operators in the Hubbard product basis; nothing here comes from the engine under test.

(i)   Engine::manyPoint (reference src/Engine/Engine.h:341-389) as the chain of obs_reference.acc_modified_state_ through the sectors, the first
      listed operator first.  One stated deviation from the reference: n and sz act in the sector the string has reached (getNeededBasis :397-400
      hands them the original sector's basis even after the string has left it, which ranks words of another particle number).
(ii)  ModelBase::rahulMethod (src/Engine/ModelBase.h:89-141) with RahulOperator::actOn (RahulOperator.h:26-50), line by line, vectorised over the kets.
(iii) for strings of c / c-dagger only: dense products of the textbook Jordan-Wigner operators of obs_reference.jordan_wigner, an independent check of (ii).
"""
from math import comb

import numpy as np

import oracle
import obs_reference as ref

UP, DOWN = 0, 1


def parse(text):
    """the -M text of LanczosDriver1.h:24-40"""
    out = []
    for tok in text.split(";"):
        p = tok.split("?")
        out.append((p[0], int(p[1]), int(p[2])))
    return out


def size(L, parts):
    return comb(L, parts[0]) * comb(L, parts[1])


# ---- (i) ---------------------------------------------------------------------------------------------------------------------------------
def chain(ops, L, parts, ket, factor=1.0):
    """(O_{n-1} ... O_0 ket, final parts), or (None, None) where hasNewParts answers false on the way"""
    cur, p = np.array(ket, copy=True), tuple(parts)
    for k, (op, site, spin) in enumerate(ops):
        newp = ref.new_sector(op, spin, L, p[0], p[1])
        if newp is None:
            return None, None
        z = np.zeros(size(L, newp), cur.dtype)
        ref.acc_modified_state_(z, op, L, p, tuple(newp), cur, site, spin, factor if k == 0 else 1.0)
        cur, p = z, tuple(newp)
    return cur, p


def many_point(ops, L, parts, bra, ket):
    v, p = chain(ops, L, parts, ket)
    if v is None or tuple(p) != tuple(parts):
        return 0.0
    return np.vdot(bra, v)


def chain_action(ops, L, parts):
    """the chain as one map: for every ket of `parts` the index it ends at in the final sector (or -1) and the coefficient; (None, None, None) for no sector"""
    n = size(L, parts)
    idx, coef, p = np.arange(n, dtype=np.int64), np.ones(n), tuple(parts)
    for op, site, spin in ops:
        newp = ref.new_sector(op, spin, L, p[0], p[1])
        if newp is None:
            return None, None, None
        i2, c2 = ref.action(op, L, p, tuple(newp), site, spin)
        live = idx >= 0
        safe = np.where(live, idx, 0)
        coef = np.where(live, coef * c2[safe], 0.0)
        idx = np.where(live, i2[safe], -1)
        coef = np.where(idx >= 0, coef, 0.0)
        p = tuple(newp)
    return idx, coef, p


# ---- (ii) --------------------------------------------------------------------------------------------------------------------------------
def _act_on(label, transpose, bit):
    """RahulOperator::actOn over an array of bits: (nonZero, new bit, result)"""
    one = np.ones(len(bit))
    if label == "identity":
        return np.ones(len(bit), bool), bit, one
    if label == "n":
        return bit.copy(), bit, one
    if label == "sz":
        return np.ones(len(bit), bool), bit, np.where(bit, -0.5, 0.5)
    if label == "c":
        return (bit & (not transpose)) | (~bit & bool(transpose)), ~bit, one
    raise RuntimeError("RahulOperator: Unknow label " + label)


def rahul_method(vops, L, parts, psi):
    """psiNew of ModelBase::rahulMethod; vops = [(label, site, dof, transpose)], the LAST acts first.  Raises where a surviving word leaves the basis."""
    ket1, ket2 = oracle.hubbard_basis_words(L, parts[0], parts[1])
    b1, b2 = ref._species_basis(L, parts[0]), ref._species_basis(L, parts[1])
    value = np.array(psi, copy=True)
    kp = [ket1.copy(), ket2.copy()]
    alive = np.ones(len(ket1), bool)
    for label, site, dof, transpose in reversed(vops):
        mask = np.uint64(1 << site)
        sbit = (kp[dof] & mask) > 0
        non_zero, new_bit, result = _act_on(label, transpose, sbit)
        kp[dof] = np.where(non_zero & (new_bit != sbit), kp[dof] ^ mask, kp[dof])  # applyOperator :165-179
        alive &= non_zero
        if label == "c":  # isFermionic
            over_up = ref.popcount(kp[UP]) if dof == DOWN else np.zeros(len(ket1), np.int64)
            result = np.where(over_up & 1, -result, result)
            result = result * ref._pg_do_sign(kp[dof], site)
        value = value * result
    out = np.zeros(len(ket1), value.dtype)
    if np.any(alive):
        w1, w2 = kp[UP][alive], kp[DOWN][alive]
        if np.any(ref.popcount(w1) != parts[0]) or np.any(ref.popcount(w2) != parts[1]):
            raise RuntimeError("rahulMethod: perfectIndex of a word outside the basis")
        new_i = ref._perfect_index(b1, w1) + ref._perfect_index(b2, w2) * len(b1)
        np.add.at(out, new_i, value[alive])
    return out


def measure(vops, L, parts, bra, ket):
    return np.vdot(bra, rahul_method(vops, L, parts, ket))


# ---- (iii) -------------------------------------------------------------------------------------------------------------------------------
def jordan_wigner_product(vops, L, parts, psi):
    """the same vector for a string of c / c-dagger only, as a product of dense Jordan-Wigner matrices through the sectors (the last acts first)"""
    cur, p = np.array(psi, copy=True), tuple(parts)
    for label, site, dof, transpose in reversed(vops):
        assert label == "c"
        op = "cdagger" if transpose else "c"
        d = 1 if transpose else -1
        newp = (p[0] + d, p[1]) if dof == UP else (p[0], p[1] + d)
        if min(newp) < 0 or max(newp) > L:
            return np.zeros(size(L, parts), cur.dtype)
        index, sign = ref.jordan_wigner(op, L, p, newp, site, dof)
        m = np.zeros((size(L, newp), size(L, p)))
        ok = index >= 0
        m[index[ok], np.nonzero(ok)[0]] = sign[ok]
        cur, p = m @ cur, newp
    assert p == tuple(parts)
    return cur


# ---- the engine's plan in the oracle's form ----------------------------------------------------------------------------------------------
def plan_action(plan, L, parts):
    """lanczosplusplus_amd.operator_string_plan turned into the form of chain_action: for every ket of `parts` the destination index (or -1) and the
    coefficient (signs of the two tables, the sz factors on the SOURCE words, the scale)"""
    tu, td = plan["table_up"].astype(np.int64), plan["table_down"].astype(np.int64)
    nu_src = comb(L, parts[0])
    n_src = nu_src * comb(L, parts[1])
    index, coef = np.full(n_src, -1, np.int64), np.zeros(n_src)
    du, dd = np.meshgrid(np.arange(len(tu)), np.arange(len(td)))  # dd major
    du, dd = du.ravel(), dd.ravel()
    m = (tu[du] != 0) & (td[dd] != 0)
    du, dd = du[m], dd[m]
    su, sd = np.abs(tu[du]) - 1, np.abs(td[dd]) - 1
    c = np.sign(tu[du]) * np.sign(td[dd]) * plan["scale"]
    wu, wd = ref._species_basis(L, parts[0])[su].astype(np.int64), ref._species_basis(L, parts[1])[sd].astype(np.int64)
    for site, fu, fd in plan["sz"]:
        c = c * ((((wu >> site) & 1) ^ fu) - (((wd >> site) & 1) ^ fd))
    keep = c != 0
    src = su[keep] + sd[keep] * nu_src
    assert len(np.unique(src)) == len(src)
    index[src] = du[keep] + dd[keep] * len(tu)
    coef[src] = c[keep]
    return index, coef
