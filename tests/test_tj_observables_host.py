"""Host side of the t-J observables (no GPU): sector arithmetic and the expanded operator plan -- expanded through the tables and the lookup function
the kernel uses -- against the literal restatement in tests/tj_obs_reference.py, which searches the sorted word list and knows no factorisation."""
import numpy as np
import pytest

import tj_obs_reference as ref
from lanczosplusplus_amd import LppError, new_parts, operator_plan_tj

# (L; nup, ndown): the sectors the factorisation was first checked in, (8;3,3), (8;4,4) (no holes: cdagger has no sector), and an empty species each way
SECTORS = [(4, (1, 1)), (5, (2, 1)), (5, (1, 3)), (6, (2, 2)), (6, (3, 3)), (6, (1, 2)), (7, (2, 1)), (8, (3, 3)), (8, (4, 4)), (7, (2, 0)), (7, (0, 2))]


@pytest.mark.parametrize("op", ref.OPS)
def test_sector_arithmetic(op):
    """TjMultiOrb::hasNewParts for every operator, both spins, L = 4, every sector with nup + ndown <= L ((0,0) included); more electrons than sites is
    no sector of this basis"""
    L = 4
    for spin in (ref.UP, ref.DOWN):
        for nup in range(L + 1):
            for ndown in range(L + 1 - nup):
                if op in ("n", "sz"):  # the reference throws
                    with pytest.raises(LppError) as ei:
                        new_parts(op, spin, L, nup, ndown, basis="tj")
                    assert ei.value.status == 1
                    with pytest.raises(RuntimeError):
                        ref.has_new_parts(op, spin, L, nup, ndown)
                    continue
                assert new_parts(op, spin, L, nup, ndown, basis="tj") == ref.has_new_parts(op, spin, L, nup, ndown), (op, spin, nup, ndown)
    with pytest.raises(LppError) as ei:
        new_parts("c", 0, L, 3, 2, basis="tj")
    assert ei.value.status == 1
    assert new_parts("cdagger", 0, L, 2, 2, basis="tj") is None and new_parts("cdagger", 1, L, 1, 3, basis="tj") is None  # nup + ndown > L
    assert new_parts("c", 0, L, 1, 0, basis="tj") is None and new_parts("c", 1, L, 0, 1, basis="tj") is None  # (0,0)
    assert new_parts("c", 0, L, 0, 0, basis="tj") is None and new_parts("cdagger", 0, L, 0, 0, basis="tj") == (1, 0)
    assert new_parts("splus", 0, L, 0, 0, basis="tj") is None and new_parts("sminus", 1, L, 0, 0, basis="tj") is None
    assert new_parts("splus", 0, L, 1, 2, basis="tj") == (2, 1) and new_parts("splus", 1, L, 1, 2, basis="tj") == (0, 3)  # the spin is read
    assert new_parts("cdagger", 0, L, 2, 2) == (3, 2)  # the default basis is unchanged


@pytest.mark.parametrize("op", ref.OPS)
@pytest.mark.parametrize("L,parts", SECTORS)
def test_plan_against_word_search(op, L, parts):
    """action[dst] = +-(src + 1) equals the restatement's (index, sign) list exactly: every site, both spins (UP only for splus / sminus)"""
    n_src = ref.size(L, *parts)
    touched = 0
    for spin in ((ref.UP,) if op in ("splus", "sminus") else (ref.UP, ref.DOWN)):
        want_parts = ref.new_sector(op, spin, L, *parts)
        for site in range(L):
            plan = operator_plan_tj(op, site, spin, L, *parts)
            if want_parts is None:
                assert plan is None
                continue
            assert (plan["nup"], plan["ndown"]) == want_parts and len(plan["action"]) == ref.size(L, *want_parts)
            idx_r, coef_r = ref.action(op, L, parts, want_parts, site, spin)
            idx_p, coef_p = ref.plan_action(plan, n_src)
            assert np.array_equal(idx_p, idx_r), (op, spin, site)  # same destination, same set of touched entries
            m = idx_r >= 0
            assert np.array_equal(coef_p[m], coef_r[m]), (op, spin, site)  # same sign
            touched += int(m.sum())
    if sum(parts) == L and op == "cdagger":
        assert touched == 0 and ref.new_sector(op, ref.UP, L, *parts) is None and ref.new_sector(op, ref.DOWN, L, *parts) is None  # no holes
    elif 0 not in parts:  # (with an empty species some operators have nothing to act on)
        assert touched > 0


def test_splus_sminus_spin_down_refused():
    """hasNewParts names (nup -+ 1, ndown +- 1) while getBraIndex ignores the spin: the reference ranks words outside the basis; the plan refuses"""
    for L, parts in SECTORS:
        for op in ("splus", "sminus"):
            with pytest.raises(LppError) as ei:
                operator_plan_tj(op, 0, ref.DOWN, L, *parts)
            assert ei.value.status == 1 and "spin DOWN" in str(ei.value)
    # ... and the restatement shows why, in a sector where hasNewParts answers
    L, parts = 6, (2, 2)
    named = ref.has_new_parts("splus", ref.DOWN, L, *parts)
    assert named == (1, 3)
    with pytest.raises(ref.NotInBasis):
        ref.action("splus", L, parts, named, 0, ref.DOWN)


def test_bad_arguments():
    for args in (("c", 0, 0, 4, 3, 2), ("c", 4, 0, 4, 1, 1), ("c", -1, 0, 4, 1, 1), ("c", 0, 2, 4, 1, 1), ("c", 0, 0, 31, 1, 1)):
        with pytest.raises(LppError) as ei:
            operator_plan_tj(*args)
        assert ei.value.status == 1, args


def test_c_down_is_jordan_wigner_at_every_site():
    """c, spin down, L = 6 (3,3), up orbitals before down: doSignGf carries the up parity at site 0 too -- no site-0 quirk as in the Hubbard basis"""
    L, parts = 6, (3, 3)
    new = ref.has_new_parts("c", ref.DOWN, L, *parts)
    assert new == (3, 2)
    for site in (0, 2):
        idx_j, sign_j = ref.jordan_wigner_c_down(L, parts, new, site)
        for idx, coef in (ref.action("c", L, parts, new, site, ref.DOWN), ref.plan_action(operator_plan_tj("c", site, ref.DOWN, L, *parts), ref.size(L, *parts))):
            assert np.array_equal(idx, idx_j)
            m = idx >= 0
            assert m.any() and np.array_equal(coef[m], sign_j[m]), site
