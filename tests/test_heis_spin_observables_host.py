"""Host side of the spin-S Heisenberg observables (no GPU): sector arithmetic, refusals and the expanded operator plan -- expanded through the run table
and the lookup function the kernel uses -- against the literal restatement in tests/heis_spin_obs_reference.py, which lists the digit words by
recursion, finds indices in a dictionary and knows no runs."""
import numpy as np
import pytest

import heis_spin_obs_reference as ref
from lanczosplusplus_amd import LppError, new_parts, operator_plan_heis_spin
from lanczosplusplus_amd.engine import sector_size

# (L; twiceS; szPlusConst) -> (states, lb): 45 is odd and one run; (9;2;8) has sites on both sides of the cut at lb = 6; twiceS = 3 is an odd spin whose
# every code is valid; twiceS = 4 has 3-bit digits whose codes 5-7 never occur (lb = 4); (24;2;3) has 18 high digits and few feasible high strings;
# (6;2;0) and (6;2;12) are the one-state ends
SECTORS = {(5, 2, 4): (45, 5), (9, 2, 8): (2907, 6), (8, 3, 12): (8092, 6), (7, 4, 13): (7875, 4), (5, 7, 17): (2460, 4), (24, 2, 3): (2576, 6),
           (6, 2, 0): (1, 6), (6, 2, 12): (1, 6)}


@pytest.mark.parametrize("sector", sorted(SECTORS))
def test_state_counts(sector):
    L, t, m = sector
    assert ref.size(L, t, m) == SECTORS[sector][0] == sector_size(L, m, 0, basis="spin", twiceS=t)


@pytest.mark.parametrize("op", ref.ALL_OPS)
@pytest.mark.parametrize("twiceS", [1, 2, 3, 4])
def test_sector_arithmetic(op, twiceS):
    """the new sector for every operator, both spins, every szPlusConst of L = 4: (szPlusConst +- 1, 0), None for sz, and LPP_ERR_INVALID -- not "no
    sector" -- for S+ on the top sector, S- on szPlusConst = 0, n, c and cdagger"""
    L = 4
    for spin in (0, 1):
        for m in range(L * twiceS + 1):
            try:
                want = ref.has_new_parts(op, L, twiceS, m, spin)
            except ref.Refused:
                with pytest.raises(LppError) as ei:
                    new_parts(op, spin, L, m, 0, basis="spin", twiceS=twiceS)
                assert ei.value.status == 1, (op, spin, m)
                continue
            got = new_parts(op, spin, L, m, 0, basis="spin", twiceS=twiceS)
            assert got == (None if want is None else (want, 0)), (op, spin, m)
    for bad in (("splus", L * twiceS), ("sminus", 0), ("n", 3), ("c", 3), ("cdagger", 3)):  # what is refused, spelled out
        with pytest.raises(ref.Refused):
            ref.has_new_parts(bad[0], L, twiceS, bad[1])
        with pytest.raises(LppError) as ei:
            new_parts(bad[0], 0, L, bad[1], 0, basis="spin", twiceS=twiceS)
        assert ei.value.status == 1


def test_refusals():
    # spins the assembler refuses: odd twiceS with twiceS + 1 no power of two; bits * L > 62; twiceS < 1
    for L, t, m in ((4, 5, 3), (4, 9, 3), (32, 2, 3), (21, 7, 3), (4, 0, 0)):
        with pytest.raises(ref.Refused):
            ref.bits_of(L, t)
        with pytest.raises(LppError) as ei:
            operator_plan_heis_spin("sz", 0, L, t, m)
        assert ei.value.status == 1, (L, t, m)
        with pytest.raises(LppError) as ei:
            new_parts("splus", 0, L, m, 0, basis="spin", twiceS=t)
        assert ei.value.status == 1, (L, t, m)
    # a site outside the chain, a digit sum outside the sector range, the operators of other models
    for args in (("sz", 6, 6, 2, 3), ("sz", -1, 6, 2, 3), ("sz", 0, 6, 2, 13), ("sz", 0, 6, 2, -1), ("n", 0, 6, 2, 3), ("c", 0, 6, 2, 3), ("cdagger", 0, 6, 2, 3),
                 ("splus", 0, 6, 2, 12), ("sminus", 0, 6, 2, 0)):
        with pytest.raises(LppError) as ei:
            operator_plan_heis_spin(*args)
        assert ei.value.status == 1, args
    with pytest.raises(LppError) as ei:
        new_parts("splus", 2, 6, 3, 0, basis="spin", twiceS=2)  # the spin is checked to be 0 or 1 ...
    assert ei.value.status == 1
    assert new_parts("splus", 1, 6, 3, 5, basis="spin", twiceS=2) == (4, 0)  # ... and otherwise not read, nor is ndown
    with pytest.raises(ValueError):
        new_parts("splus", 0, 6, 3, 0, basis="spin")  # twiceS is required
    with pytest.raises(ValueError):
        new_parts("sz", 0, 6, 3, 0, basis="heisenberg")  # stays no basis at all
    assert new_parts("cdagger", 0, 6, 2, 2) == (3, 2) and new_parts("splus", 0, 6, 3, 0, basis="spin_half") == (4, 0)  # the others are unchanged


@pytest.mark.parametrize("op", ref.OPS)
@pytest.mark.parametrize("sector", sorted(SECTORS))
def test_plan_against_dictionary_search(op, sector):
    """action[dst] = src + 1 and coef[dst] equal the restatement's (index, value) list exactly: every site"""
    L, t, m = sector
    states, lb = SECTORS[sector]
    n_src = ref.size(L, t, m)
    assert n_src == states
    try:
        new_m = ref.new_sector(op, L, t, m)
    except ref.Refused:
        for site in range(L):
            with pytest.raises(LppError) as ei:
                operator_plan_heis_spin(op, site, L, t, m)
            assert ei.value.status == 1
        return
    sides = set()
    for site in range(L):
        plan = operator_plan_heis_spin(op, site, L, t, m)
        assert (plan["nup"], plan["ndown"]) == (new_m, 0) and len(plan["action"]) == len(plan["coef"]) == ref.size(L, t, new_m)
        assert plan["lb"] == lb
        sides.add(site < plan["lb"])
        idx_r, val_r = ref.action(op, L, t, m, site)
        idx_p, coef_p = ref.plan_action(plan, n_src)
        live = (idx_r >= 0) & (val_r != 0)  # a value of 0 leaves the destination untouched
        assert np.array_equal(idx_p >= 0, live), (op, site)
        assert np.array_equal(idx_p[live], idx_r[live]), (op, site)  # same destination, same set of touched entries
        assert np.array_equal(coef_p[live], val_r[live]), (op, site)  # the host table's double
        assert np.array_equal(np.nonzero(plan["action"])[0], np.nonzero(ref.touched(op, L, t, m, site))[0]), (op, site)
    assert sides == ({True, False} if L > lb else {True})  # sites on both sides of the cut were covered


def test_both_sides_of_the_cut_are_in_the_sectors():
    assert sum(L > lb for (L, _, _), (_, lb) in SECTORS.items()) >= 5 and any(L <= lb for (L, _, _), (_, lb) in SECTORS.items())


def test_twice_s_one_is_the_spin_half_plan():
    """twiceS = 1 through the digit planner: the S = 1/2 plan's sources, splus / sminus with value 1, sz with value bit - 1/2"""
    from lanczosplusplus_amd import operator_plan_heis
    L, m = 14, 6  # 14 one-bit digits: two above the cut of 12
    for site in (0, 11, 12, 13):
        for op in ("splus", "sminus", "sz"):
            a = operator_plan_heis(op, site, 0, L, m)
            b = operator_plan_heis_spin(op, site, L, 1, m)
            assert b["lb"] == a["lb"] == 12 and b["nup"] == a["nup"]
            assert np.array_equal(np.abs(a["action"]), b["action"]), (op, site)
            want = -0.5 * np.sign(a["action"]) if op == "sz" else (a["action"] != 0).astype(float)
            assert np.array_equal(b["coef"], want), (op, site)


def test_long_chain_plans_from_the_feasible_high_strings():
    """24 sites with digit sum 3: 2576 states; the plan walks the high strings that can occur, not the 3^18 of the high part"""
    import time
    t0 = time.perf_counter()
    plan = operator_plan_heis_spin("sz", 23, 24, 2, 3)
    assert len(plan["action"]) == 2576 and plan["lb"] == 6
    assert time.perf_counter() - t0 < 2.0  # (milliseconds; walking 3^18 strings takes many seconds)
    # S = 1, 20 sites, Sz = 0: 4.6e6 runs at 12 bits pass the run table's limit, 14 bits hold; 31 sites pass it at 14 as well
    from lanczosplusplus_amd import _capi
    import ctypes as C
    has, m2, n, lb = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
    st = _capi.lib().lpp_obs_plan_heis_spin(2, 0, 0, 20, 2, 20, C.byref(has), C.byref(m2), C.byref(n), C.byref(lb), None, None)
    assert st == 0 and lb.value == 7 and n.value == 377379369
    with pytest.raises(LppError) as ei:
        operator_plan_heis_spin("sz", 0, 31, 2, 31)
    assert ei.value.status == 1 and "runs" in str(ei.value)


def test_planner_under_sanitizers(tmp_path):
    """the digit-basis planner in a stand-alone program (its own main) built with the address and undefined-behaviour sanitizers: it plans and expands
    the sectors above and the planner's limits, checks sources, touched counts and a brute-force word list; the program prints `ok`"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "lanczosplusplus_amd", "host", "test_heis_spin_plan.cpp")
    exe = str(tmp_path / "test_heis_spin_plan")
    out = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "lanczosplusplus_amd", "csrc"), "-o", exe, src],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout
