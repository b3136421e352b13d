"""Host side of the operator strings in the one-orbital t-J basis (no GPU): the composed plan of a string -- a few words, one entry per destination
down word and a program of pattern steps, expanded through the lookup function the kernels use -- against the chain of accModifiedState_ steps in
tests/tj_many_point_reference.py, which searches the sorted word list and knows neither patterns nor masks nor tables."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tj_many_point_reference as mp
import tj_obs_reference as ref
from lanczosplusplus_amd import LppError, _capi, operator_plan_tj, operator_string_plan_tj
from tj_many_point_reference import DOWN, UP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (L; nup, ndown): 105 states, odd, blocks of 5; (7;2,2); 4200 states; (9;1,3); one block; blocks of one element; full: cdagger finds no sector
SECTORS = [(7, 1, 2), (7, 2, 2), (10, 3, 3), (9, 1, 3), (8, 3, 0), (9, 0, 3), (6, 3, 3)]
# destinations reached by strings 0-8, 13 and 14 (worked out on the restatement; conditions, not measurements)
REACHED = {(7, 1, 2): [5, 15, 10, 20, 3, 5, 5, 15, 15, 15, 0], (7, 2, 2): [20, 60, 30, 30, 6, 20, 20, 60, 60, 60, 4],
           (10, 3, 3): [420, 1260, 560, 560, 90, 420, 420, 1260, 1260, 1260, 105]}
STAYING = {(7, 1, 2): 10, (7, 2, 2): 11, (10, 3, 3): 11}


@pytest.mark.parametrize("L,nup,ndown", SECTORS)
def test_plan_against_the_chain(L, nup, ndown):
    """every string: the expanded action word by word, the final sector, the dead flag, the closed-form count; and the words evaluated directly"""
    parts = (nup, ndown)
    n_src = ref.size(L, *parts)
    nonzero, reached = 0, []
    for k, string in enumerate(mp.strings(L)):
        want, new = mp.action(string, L, parts)
        plan = operator_string_plan_tj(string, L, nup, ndown)
        if want is None:
            assert plan is None, k
            continue
        assert plan is not None and (plan["nup"], plan["ndown"]) == new and plan["n_dst"] == len(want) == ref.size(L, *new), k
        assert np.array_equal(plan["action"], want), k
        assert plan["touched"] == np.count_nonzero(want), k
        assert np.all(np.abs(plan["action"]) <= n_src)
        assert plan["dead"] or want.any() or plan["touched"] == 0, k
        if plan["dead"]:
            assert not want.any(), k
        assert operator_string_plan_tj(mp.text(string), L, nup, ndown, action=False) == {key: v for key, v in plan.items() if key != "action"}
        if k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 13, 14):
            reached.append(np.count_nonzero(want))
        if plan["dead"]:
            continue
        # the words on the destination words: us = u ^ flip_up, ds = d ^ flip_down, conditions and parities on the source
        _, u, d = ref.basis(L, *new)
        us, ds = u ^ np.uint64(plan["flip_up"]), d ^ np.uint64(plan["flip_down"])
        ok = ((us & np.uint64(plan["mask"])) == np.uint64(plan["want_up"])) & ((ds & np.uint64(plan["mask"])) == np.uint64(plan["want_down"]))
        par = (ref.popcount(us & np.uint64(plan["par_up"])) + ref.popcount(ds & np.uint64(plan["par_down"]))) & 1
        direct = np.zeros(len(u), np.int64)
        assert not np.any(us[ok] & ds[ok])  # (every source that passes is a basis word)
        if ok.any():
            direct[ok] = plan["sign"] * (1 - 2 * par[ok]) * (ref.perfect_index(L, parts, us[ok], ds[ok]) + 1)
        assert np.array_equal(direct, want), k
        nonzero += bool(want.any()) and new == parts
    if (L,) + parts in REACHED:
        assert reached == REACHED[(L,) + parts]
        assert nonzero >= STAYING[(L,) + parts]


@pytest.mark.parametrize("L,nup,ndown", [(7, 2, 2), (8, 3, 0), (9, 0, 3), (6, 3, 3), (9, 1, 3)])
def test_length_one_strings_are_the_operator_plans(L, nup, ndown):
    for op in ref.OPS:
        for spin in (UP, DOWN):
            if op in ("splus", "sminus") and spin == DOWN:
                continue
            for site in sorted({0, 3, L // 2, L - 1}):
                one = operator_plan_tj(op, site, spin, L, nup, ndown)
                plan = operator_string_plan_tj([(op, site, spin)], L, nup, ndown)
                assert (one is None) == (plan is None), (op, site, spin)
                if one is None:
                    continue
                assert (plan["nup"], plan["ndown"]) == (one["nup"], one["ndown"]) and not plan["dead"]
                assert np.array_equal(plan["action"], one["action"]), (op, site, spin)
                assert plan["touched"] == np.count_nonzero(one["action"])


def test_the_zero_zero_walk():
    """c then cdagger of the only electron: the (0,0) sector does not exist (TjMultiOrb::hasNewParts)"""
    assert mp.action([("c", 0, UP), ("cdagger", 0, UP)], 5, (1, 0)) == (None, None)
    assert operator_string_plan_tj([("c", 0, UP), ("cdagger", 0, UP)], 5, 1, 0) is None
    assert operator_string_plan_tj([("c", 0, UP), ("c", 0, UP)], 7, 1, 2) is None  # string 9 with one up electron


def test_refusals():
    for string, L, nup, ndown in (([("n", 7, UP)], 7, 2, 2), ([("n", 0, UP), ("c", -1, DOWN)], 7, 2, 2), ([], 7, 2, 2), ([("n", 0, UP)] * 17, 7, 2, 2),
                                  ([("n", 0, UP)], 7, 4, 4), ([("n", 0, UP)], 31, 2, 2), ([("n", 0, UP)], 7, -1, 2), ([("n", 0, 2)], 7, 2, 2),
                                  ([("splus", 0, DOWN)], 7, 2, 2), ([("n", 0, UP), ("sminus", 1, DOWN)], 7, 2, 2),
                                  ([("c", 0, UP), ("cdagger", 1, UP)], 26, 1, 1)):  # 25 sites free of down electrons and a change of the pattern
        with pytest.raises(LppError) as ei:
            operator_string_plan_tj(string, L, nup, ndown)
        assert ei.value.status == 1, string
    # (26;1,1), 650 states: a string that does not change the pattern is planned
    plan = operator_string_plan_tj([("n", 0, DOWN)], 26, 1, 1)
    assert plan["n_dst"] == 650 and plan["touched"] == 25 == np.count_nonzero(plan["action"])
    with pytest.raises(ValueError):
        operator_string_plan_tj([("nn", 0, UP)], 7, 2, 2)
    # the measure convention is not restated for this basis
    one = np.array([_capi.LPP_OP_N, 0, 0], np.int32)
    has = C.c_int32()
    args = [C.c_void_p(one[k:].ctypes.data) for k in (0, 1, 1, 1)] + [7, 2, 2, C.byref(has)] + [None] * 9
    assert _capi.lib().lpp_obs_string_plan_tj(_capi.LPP_STRING_MANY_POINT, 1, *args) == 0 and has.value == 1
    with pytest.raises(LppError) as ei:
        _capi.check(_capi.lib().lpp_obs_string_plan_tj(_capi.LPP_STRING_MEASURE, 1, *args))
    assert ei.value.status == 1 and "many-point" in str(ei.value)


def test_planner_under_sanitizers(tmp_path):
    """the host planner in a stand-alone program (its own main) built with the address and undefined-behaviour sanitizers: the strings of this file on the
    seven sectors against a chain of one-operator plans (obs_plan_tj + tj_expand), the packer's refusals, batches of 1, 8 and 5 read back against
    their plans, and planning alone at 30 sites; the program prints `ok`"""
    src = os.path.join(ROOT, "lanczosplusplus_amd", "host", "test_tj_string_plan.cpp")
    exe = str(tmp_path / "test_tj_string_plan")
    out = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                          "-I" + os.path.join(ROOT, "lanczosplusplus_amd", "csrc"), "-o", exe, src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout
