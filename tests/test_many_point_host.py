"""Host side of the operator strings (no GPU): lanczosplusplus_amd.operator_string_plan turned into (index, coefficient) per ket against the chained
oracle of tests/many_point_reference.py (many-point convention) and against the literal rahulMethod and dense Jordan-Wigner products (measure convention)."""
import os
import subprocess

import numpy as np
import pytest

import many_point_reference as mp
import obs_reference as ref
import oracle
from lanczosplusplus_amd import LppError, operator_plan, operator_string_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP, DOWN = ref.UP, ref.DOWN

PAIR = [("c", 1, UP), ("c", 2, DOWN), ("cdagger", 4, DOWN), ("cdagger", 3, UP)]  # pair hopping: ends in the sector it started in
LONG16 = [("c", 0, UP), ("n", 3, UP), ("cdagger", 5, UP), ("sz", 5, UP), ("splus", 2, UP), ("sz", 2, UP), ("sminus", 2, UP), ("c", 0, DOWN),
          ("c", 4, DOWN), ("n", 1, UP), ("cdagger", 0, DOWN), ("sz", 0, DOWN), ("cdagger", 4, DOWN), ("c", 5, UP), ("cdagger", 0, UP), ("n", 0, UP)]


def _check_string(ops, L, parts):
    idx_r, coef_r, parts_r = mp.chain_action(ops, L, parts)
    plan = operator_string_plan(ops, L, *parts)
    if idx_r is None:
        assert plan is None
        return None
    assert plan is not None and (plan["nup"], plan["ndown"]) == parts_r and plan["scale"] == 1.0
    idx_t, coef_t = mp.plan_action(plan, L, parts)
    assert np.array_equal(idx_t, idx_r), ops  # same destinations, same set of surviving kets
    assert np.array_equal(coef_t[idx_r >= 0], coef_r[idx_r >= 0]), ops
    return plan


def test_chain_action_is_the_chain():
    """the oracle's own two forms agree: the composed map applied to a random vector is the chain of accModifiedState_"""
    L, parts = 6, (3, 3)
    ket = oracle.fill_random(mp.size(L, parts), 11)
    for ops in (PAIR, LONG16, [("sz", 1, UP), ("c", 1, UP), ("sz", 1, DOWN)]):
        v, p = mp.chain(ops, L, parts, ket)
        idx, coef, p2 = mp.chain_action(ops, L, parts)
        assert p == p2
        z = np.zeros(mp.size(L, p))
        m = idx >= 0
        np.add.at(z, idx[m], coef[m] * ket[m])
        assert np.array_equal(z, v)


@pytest.mark.parametrize("op", ref.OPS)
@pytest.mark.parametrize("L,parts", [(6, (3, 3)), (6, (2, 4)), (5, (2, 1)), (6, (3, 0)), (6, (0, 3))])
def test_length_one_reproduces_operator_plan(op, L, parts):
    for spin in (UP, DOWN):
        for site in range(L):
            plan = _check_string([(op, site, spin)], L, parts)
            one = operator_plan(op, site, spin, L, *parts)
            assert (plan is None) == (one is None)
            if plan is None:
                continue
            assert (plan["nup"], plan["ndown"]) == (one["nup"], one["ndown"])
            if op == "sz":  # operator_plan hands out the two occupancy tables, the string plan the identity and one sz entry
                assert plan["sz"] == [(site, 0, 0)]
                assert np.array_equal(plan["table_up"], np.arange(1, len(plan["table_up"]) + 1))
            else:
                assert plan["sz"] == []
                assert np.array_equal(plan["table_up"], one["table_up"]) and np.array_equal(plan["table_down"], one["table_down"])


@pytest.mark.parametrize("L,parts", [(6, (3, 3)), (6, (2, 4)), (5, (2, 1)), (8, (4, 3))])
def test_strings_against_the_chain(L, parts):
    two = [[("c", 0, UP), ("cdagger", 2, UP)], [("cdagger", 1, DOWN), ("c", 0, DOWN)], [("n", 0, UP), ("n", 1, DOWN)], [("splus", 1, UP), ("sminus", 3, UP)],
           [("c", 0, DOWN), ("sz", 0, UP)], [("sz", 2, DOWN), ("cdagger", 2, UP)], [("c", 2, UP), ("c", 2, UP)]]
    four = [PAIR, [("c", 0, DOWN), ("c", 1, UP), ("cdagger", 0, DOWN), ("cdagger", 1, UP)], [("n", 0, UP), ("n", 1, UP), ("n", 2, DOWN), ("n", 0, DOWN)],
            [("splus", 0, UP), ("c", 1, UP), ("sminus", 0, DOWN), ("cdagger", 3, UP)]]
    sz2 = [[("sz", 0, UP), ("sz", 1, UP)], [("sz", 1, UP), ("c", 1, UP), ("sz", 1, UP), ("cdagger", 1, UP)], [("sminus", 2, UP), ("sz", 2, UP), ("splus", 2, UP), ("sz", 2, UP)]]
    sz3 = [[("sz", 0, UP), ("sz", 0, UP), ("sz", 3, DOWN)], [("sz", 1, UP), ("c", 1, DOWN), ("sz", 1, UP), ("cdagger", 0, UP), ("sz", 0, DOWN)]]
    for ops in two + four + sz2 + sz3:
        _check_string(ops, L, parts)
    _check_string([(op, s if s < L else L - 1, sp) for op, s, sp in LONG16], L, parts)


def test_sixteen_operators_reach_something():
    plan = _check_string(LONG16, 6, (3, 3))
    assert plan is not None and (plan["nup"], plan["ndown"]) == (3, 3) and len(plan["sz"]) == 3
    idx, _ = mp.plan_action(plan, 6, (3, 3))
    assert np.any(idx >= 0)


def test_sector_walk():
    L = 4
    # through the (0,0) sector: hasNewParts refuses it, the string has no sector
    assert _check_string([("c", 0, UP), ("cdagger", 0, UP)], L, (1, 0)) is None
    assert _check_string([("c", 1, DOWN), ("cdagger", 1, DOWN)], L, (0, 1)) is None
    # leaving [0, L]
    assert _check_string([("cdagger", 0, UP), ("c", 0, UP)], L, (4, 2)) is None
    assert _check_string([("n", 0, UP), ("c", 0, DOWN)], L, (2, 0)) is None
    assert _check_string([("splus", 0, UP)], L, (2, 0)) is None
    # ending in another sector: a plan, with other parts
    plan = _check_string([("c", 0, UP), ("n", 1, UP), ("cdagger", 2, DOWN)], L, (2, 1))
    assert (plan["nup"], plan["ndown"]) == (1, 2)
    plan = _check_string([("splus", 0, UP), ("sz", 0, DOWN)], L, (1, 2))
    assert (plan["nup"], plan["ndown"]) == (2, 1)


MEASURE = [
    [("n", 0, UP, False), ("n", 1, DOWN, False)],
    [("c", 2, UP, True), ("c", 0, UP, False)],
    [("c", 1, DOWN, True), ("c", 3, DOWN, False)],
    [("c", 3, UP, True), ("c", 4, DOWN, True), ("c", 2, DOWN, False), ("c", 1, UP, False)],
    [("sz", 0, UP, False), ("sz", 0, DOWN, False), ("identity", 2, UP, False), ("n", 1, UP, False)],
    [("c", 0, DOWN, True), ("sz", 0, DOWN, False), ("c", 0, DOWN, False), ("sz", 1, UP, False), ("sz", 1, UP, True)],
    [("c", 0, UP, False), ("c", 0, UP, True)],
    [("c", 0, UP, False), ("c", 1, DOWN, False), ("c", 2, UP, False), ("c", 2, UP, True), ("c", 1, DOWN, True), ("c", 0, UP, True), ("n", 4, DOWN, False),
     ("c", 3, DOWN, True), ("c", 3, DOWN, False), ("sz", 3, DOWN, False), ("identity", 0, DOWN, True), ("c", 4, UP, True), ("c", 4, UP, False), ("n", 4, UP, False),
     ("sz", 2, UP, False), ("n", 1, DOWN, False)],
]


@pytest.mark.parametrize("L,parts", [(6, (3, 3)), (6, (2, 3)), (5, (2, 1)), (5, (3, 2))])
def test_measure_against_rahul_method(L, parts):
    psi = oracle.fill_random(mp.size(L, parts), 21)
    for vops in MEASURE:
        plan = operator_string_plan(vops, L, *parts, convention="measure")
        assert plan is not None and (plan["nup"], plan["ndown"]) == parts and plan["sz"] == []
        assert plan["scale"] == 0.5 ** sum(1 for o in vops if o[0] == "sz")
        idx, coef = mp.plan_action(plan, L, parts)
        z = np.zeros(len(psi))
        m = idx >= 0
        np.add.at(z, idx[m], coef[m] * psi[m])
        want = mp.rahul_method(vops, L, parts, psi)
        assert np.array_equal(z, want), vops  # one product of +-1, powers of 1/2 and one vector element per entry: exact
        if all(o[0] == "c" for o in vops):
            jw = mp.jordan_wigner_product(vops, L, parts, psi)
            assert np.array_equal(want, jw), vops


def test_measure_dies_where_no_word_survives():
    """c on an empty species and back: conserving, identically zero"""
    plan = operator_string_plan([("c", 0, UP, True), ("c", 0, UP, False)], 4, 0, 2, convention="measure")
    assert plan is not None and not plan["table_up"].any()
    assert not mp.rahul_method([("c", 0, UP, True), ("c", 0, UP, False)], 4, (0, 2), np.ones(6)).any()


def test_refusals():
    with pytest.raises(ValueError):
        operator_string_plan([("cc", 0, UP)], 4, 2, 2)
    with pytest.raises(ValueError):
        operator_string_plan([("splus", 0, UP, False)], 4, 2, 2, convention="measure")
    with pytest.raises(ValueError):
        operator_string_plan([("n", 0, UP)], 4, 2, 2, convention="rahul")
    with pytest.raises(LppError):
        operator_string_plan([("n", 4, UP)], 4, 2, 2)  # site >= L
    with pytest.raises(LppError):
        operator_string_plan([("n", 0, 2)], 4, 2, 2)  # spin
    with pytest.raises(LppError):
        operator_string_plan([("n", 0, UP)] * 17, 4, 2, 2)  # more than 16 operators
    with pytest.raises(LppError):
        operator_string_plan([], 4, 2, 2)
    with pytest.raises(LppError):
        operator_string_plan([("n", 0, UP)], 4, 5, 2)  # no such sector
    with pytest.raises(LppError) as ei:
        operator_string_plan([("c", 0, UP, False)], 4, 2, 2, convention="measure")  # number changing
    assert "conserve" in str(ei.value)
    with pytest.raises(LppError):
        operator_string_plan([("c", 0, UP, True), ("c", 0, DOWN, False)], 4, 2, 2, convention="measure")  # conserves the total only
    with pytest.raises(RuntimeError):
        mp.rahul_method([("c", 0, UP, False)], 4, (2, 2), np.ones(36))  # the reference indexes outside the sector there
    assert operator_string_plan("c?0?0;cdagger?1?0", 4, 2, 2)["nup"] == 2  # the -M text


def test_planner_under_sanitizers(tmp_path):
    """the host planner in a stand-alone program (its own main) built with the address and undefined-behaviour sanitizers: the strings of this file, the
    refusals, the largest tables (L = 16, 16 operators) and the upload images of one string and of batches of 1, 8 and 5 read back against their plans,
    with a table of the wrong length refused; the program checks the tables' invariants itself and prints `ok`"""
    src = os.path.join(ROOT, "lanczosplusplus_amd", "host", "test_string_plan.cpp")
    exe = str(tmp_path / "test_string_plan")
    out = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                          "-I" + os.path.join(ROOT, "lanczosplusplus_amd", "csrc"), "-o", exe, src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout
