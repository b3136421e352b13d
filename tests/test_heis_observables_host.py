"""Host side of the S = 1/2 Heisenberg observables (no GPU): sector arithmetic and the expanded operator plan -- expanded through the run table and the
lookup function the kernel uses -- against the literal restatement in tests/heis_obs_reference.py, which searches the word list and knows no runs."""
import numpy as np
import pytest

import heis_obs_reference as ref
from lanczosplusplus_amd import LppError, new_parts, operator_plan_heis

# (L; szPlusConst): 35 states is odd; (9;0) and (9;9) are the one-state ends; 13 sites exceed the cut of the word (12 low bits by default)
SECTORS = [(6, 3), (7, 3), (9, 0), (9, 9), (12, 5), (13, 6)]


@pytest.mark.parametrize("op", ref.ALL_OPS)
def test_sector_arithmetic(op):
    """Heisenberg::hasNewParts for every operator, both spins, every szPlusConst of L = 6: the throwing ends of S+ / S- and the refusals of n, c, cdagger"""
    L = 6
    for spin in (ref.UP, ref.DOWN):
        for m in range(L + 1):
            try:
                want = ref.has_new_parts(op, spin, L, m)
            except ref.Throws:
                with pytest.raises(LppError) as ei:
                    new_parts(op, spin, L, m, 0, basis="spin_half")
                assert ei.value.status == 1, (op, spin, m)
                continue
            got = new_parts(op, spin, L, m, 0, basis="spin_half")
            assert got == (None if want is None else (want, 0)), (op, spin, m)
    # what throws, spelled out
    for bad in (("splus", L), ("sminus", 0), ("n", 3), ("c", 3), ("cdagger", 3)):
        with pytest.raises(ref.Throws):
            ref.has_new_parts(bad[0], ref.UP, L, bad[1])
    assert new_parts("sz", 0, L, 3, 0, basis="spin_half") is None
    assert new_parts("splus", 1, L, 3, 5, basis="spin_half") == (4, 0)  # neither the spin nor ndown is read
    assert new_parts("cdagger", 0, L, 2, 2) == (3, 2)  # the default basis is unchanged
    with pytest.raises(ValueError):
        new_parts("sz", 0, L, 3, 0, basis="heisenberg")


@pytest.mark.parametrize("op", ref.OPS)
@pytest.mark.parametrize("L,m", SECTORS)
def test_plan_against_word_search(op, L, m):
    """action[dst] = +-(src + 1) equals the restatement's (index, value) list exactly: every site, both spins"""
    n_src = ref.size(L, m)
    sides = set()
    for spin in (ref.UP, ref.DOWN):
        for site in range(L):
            try:
                new_m = ref.new_sector(op, spin, L, m)
            except ref.Throws:
                with pytest.raises(LppError) as ei:
                    operator_plan_heis(op, site, spin, L, m)
                assert ei.value.status == 1
                continue
            plan = operator_plan_heis(op, site, spin, L, m)
            assert (plan["nup"], plan["ndown"]) == (new_m, 0) and len(plan["action"]) == ref.size(L, new_m)
            assert plan["lb"] == min(L, 12)
            sides.add(site < plan["lb"])
            idx_r, val_r = ref.action(op, L, m, new_m, site, spin)
            idx_p, coef_p = ref.plan_action(plan, n_src)
            live = (idx_r >= 0) & (val_r != 0)  # a value of 0 leaves the destination untouched
            assert np.array_equal(idx_p >= 0, live), (op, spin, site)
            assert np.array_equal(idx_p[live], idx_r[live]), (op, spin, site)  # same destination, same set of touched entries
            assert np.array_equal(coef_p[live], val_r[live]), (op, spin, site)  # same value: +1, or -1 for sz on an up spin
    if L > 12 and not (op == "splus" and m == L) and not (op == "sminus" and m == 0):
        assert sides == {True, False}  # sites on both sides of the cut were covered


def test_refused_operators_and_bad_arguments():
    for op in ("c", "cdagger"):  # getBraIndex_ throws (:279)
        with pytest.raises(ref.Throws):
            ref.action(op, 6, 3, 3, 0, ref.UP)
        with pytest.raises(LppError) as ei:
            operator_plan_heis(op, 0, ref.UP, 6, 3)
        assert ei.value.status == 1
    # site >= L, a negative site, m > L, a bad spin, L = 63
    for args in (("sz", 6, 0, 6, 3), ("sz", -1, 0, 6, 3), ("sz", 0, 0, 6, 7), ("sz", 0, 2, 6, 3), ("sz", 0, 0, 63, 3)):
        with pytest.raises(LppError) as ei:
            operator_plan_heis(*args)
        assert ei.value.status == 1, args
    with pytest.raises(LppError) as ei:
        new_parts("splus", 0, 63, 3, 0, basis="spin_half")
    assert ei.value.status == 1


def test_long_chain_keeps_a_small_run_table():
    """62 sites, two up spins: 1891 states in 1 + 50 + 1225 runs; the plan is made from the runs that exist, not from 2^(L - lb) high parts.
    Checked against a direct enumeration of the pairs (the word list of 2^62 words cannot be searched)."""
    L, m = 62, 2
    words = np.array(sorted((1 << a) | (1 << b) for a in range(L) for b in range(a)), dtype=np.uint64)
    for site in (0, 13, 14, 40, 61):
        plan = operator_plan_heis("sz", site, ref.UP, L, m)
        assert plan["lb"] == 14 and len(plan["action"]) == len(words) == 1891
        bit = ((words >> np.uint64(site)) & np.uint64(1)).astype(np.int64)
        assert np.array_equal(plan["action"], (1 - 2 * bit) * (np.arange(len(words)) + 1)), site
        plan = operator_plan_heis("sminus", site, ref.UP, L, 3)  # destination: the pairs without the site's bit; source: the triple with it
        triples = np.array(sorted((1 << a) | (1 << b) | (1 << c) for a in range(L) for b in range(a) for c in range(b)), dtype=np.uint64)
        want = np.where(bit == 0, np.searchsorted(triples, words | np.uint64(1 << site)) + 1, 0)
        assert np.array_equal(plan["action"], want), site
        plan = operator_plan_heis("splus", site, ref.UP, L, m)  # destination: the triples with the site's bit; source: the pair without it
        tbit = ((triples >> np.uint64(site)) & np.uint64(1)).astype(np.int64)
        want = np.where(tbit == 1, np.searchsorted(words, triples & ~np.uint64(1 << site)) + 1, 0)
        assert plan["nup"] == 3 and np.array_equal(plan["action"], want), site
        for spin in (ref.UP, ref.DOWN):
            plan = operator_plan_heis("n", site, spin, L, m)
            assert np.array_equal(plan["action"], np.where(bit == (1 if spin == ref.UP else 0), np.arange(len(words)) + 1, 0)), (site, spin)
    with pytest.raises(LppError) as ei:
        operator_plan_heis("sz", 0, ref.UP, 62, 31)  # 2^48 runs: beyond the run table's index
    assert ei.value.status == 1 and "runs" in str(ei.value)
