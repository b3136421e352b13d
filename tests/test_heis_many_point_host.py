"""Host side of the operator strings in the S = 1/2 Heisenberg basis (no GPU): the composed plan of a string -- five words and a sign, expanded through
the run entries and the lookup function the kernels use -- against the chain of accModifiedState_ steps in tests/heis_many_point_reference.py, which
searches the word list and knows neither masks nor runs."""
import ctypes as C
import os
import subprocess
from itertools import combinations

import numpy as np
import pytest

import heis_many_point_reference as mp
import heis_obs_reference as ref
from heis_many_point_reference import DOWN, UP
from lanczosplusplus_amd import LppError, _capi, operator_plan_heis, operator_string_plan_heis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (L; szPlusConst): 21 states, odd, one run; (7;3); the smallest with a high part; several tiles; (16;8); 64 runs
SECTORS = [(7, 2), (7, 3), (14, 7), (16, 7), (16, 8), (18, 9)]


@pytest.mark.parametrize("L,m", SECTORS)
def test_plan_against_the_chain(L, m):
    """every string: the expanded action word by word, the final sector, the dead flag; and the words themselves evaluated directly on the word list"""
    words = ref.basis(L, m)
    nonzero = 0
    for k, string in enumerate(mp.strings(L)):
        want, new_m = mp.action(string, L, m)
        plan = operator_string_plan_heis(string, L, m)
        assert plan["szPlusConst"] == new_m and plan["n_dst"] == len(want) == ref.size(L, new_m) and plan["lb"] == min(L, 12), k
        assert plan["dead"] == (k in mp.DEAD), k
        assert (new_m != m) == (k in mp.LEAVES) or k in mp.DEAD, k  # (splus twice is dead and ends two sectors up)
        assert np.array_equal(plan["action"], want), k
        assert np.all(np.abs(plan["action"]) <= len(words))
        assert operator_string_plan_heis(mp.text(string), L, m, action=False) == {key: v for key, v in plan.items() if key != "action"}
        if plan["dead"]:
            assert not want.any()
            continue
        # the five words on the destination words: result[d] = sign * (-1)^popcount((d ^ flip) & zmask) * src[rank(d ^ flip)] where ((d ^ flip) & need) == want
        dst = ref.basis(L, new_m)
        srcw = dst ^ np.uint64(plan["flip"])
        ok = (srcw & np.uint64(plan["need"])) == np.uint64(plan["want"])
        par = np.array([bin(int(w) & plan["zmask"]).count("1") & 1 for w in srcw])
        direct = np.zeros(len(dst), np.int64)
        direct[ok] = plan["sign"] * (1 - 2 * par[ok]) * (ref.perfect_index(L, m, srcw[ok]) + 1)
        assert np.array_equal(direct, want), k
        nonzero += bool(want.any()) and new_m == m
    assert nonzero >= 10


@pytest.mark.parametrize("L,m", [(7, 3), (13, 6), (16, 8)])
def test_length_one_strings_are_the_operator_plans(L, m):
    for op in ref.OPS:
        for spin in (UP, DOWN):
            for site in sorted({0, 3, min(L, 12) - 1, min(12, L - 1), L - 1}):
                one = operator_plan_heis(op, site, spin, L, m)
                plan = operator_string_plan_heis([(op, site, spin)], L, m)
                assert plan["szPlusConst"] == one["nup"] and plan["lb"] == one["lb"] and not plan["dead"]
                assert np.array_equal(plan["action"], one["action"]), (op, site, spin)


def test_long_chain_against_direct_enumeration():
    """(40;3): 9880 words listed directly, the cut of the word at 14 bits; sites 13 | 14 straddle it"""
    L, m = 40, 3
    words = np.array(sorted(sum(1 << b for b in c) for c in combinations(range(L), m)), np.uint64)
    assert len(words) == 9880
    index = {int(w): i for i, w in enumerate(words)}
    bit = lambda w, s: (int(w) >> s) & 1  # noqa: E731
    for string in ([("sminus", 0, UP), ("splus", 39, UP)], [("sz", 13, UP), ("sz", 14, UP)], [("sminus", 13, UP), ("splus", 14, UP)]):
        plan = operator_string_plan_heis(string, L, m)
        assert plan["lb"] == 14 and plan["szPlusConst"] == m and not plan["dead"] and len(plan["action"]) == 9880
        want = np.zeros(9880, np.int64)
        for i, w in enumerate(words):  # forward from every source word
            w, c = int(w), 1
            for op, site, _ in string:
                if op == "sz":
                    c *= 1 - 2 * bit(w, site)
                elif bit(w, site) == (op == "sminus"):
                    w ^= 1 << site
                else:
                    c = 0
                    break
            if c:
                want[index[w]] = c * (i + 1)
        assert want.any() and np.array_equal(plan["action"], want), string


def test_refusals():
    for string, L, m in (([("c", 0, UP)], 7, 3), ([("sz", 0, UP), ("cdagger", 1, DOWN)], 7, 3), ([("sz", 7, UP)], 7, 3), ([], 7, 3), ([("sz", 0, UP)] * 17, 7, 3),
                         ([("splus", 0, UP)], 4, 4), ([("sminus", 0, UP)], 4, 0), ([("sminus", 0, UP), ("sminus", 1, UP)], 4, 1), ([("sz", 0, UP)], 7, 8)):
        with pytest.raises(LppError) as ei:
            operator_string_plan_heis(string, L, m)
        assert ei.value.status == 1, string
    # ... at the second step: the first alone is served, and so is the reference chain
    assert operator_string_plan_heis([("sminus", 0, UP)], 4, 1)["szPlusConst"] == 0
    with pytest.raises(mp.Throws):
        mp.apply_string([("sminus", 0, UP), ("sminus", 1, UP)], 4, 1, np.ones(4))
    # a dead string still walks the sectors: splus twice on one site of the sector below the full one
    with pytest.raises(LppError):
        operator_string_plan_heis([("splus", 0, UP), ("splus", 0, UP)], 4, 3)
    with pytest.raises(ValueError):
        operator_string_plan_heis([("nn", 0, UP)], 7, 3)
    # the measure convention is not for the spin basis (the engine's methods: tests/test_gpu_heis_many_point.py)
    one = np.array([_capi.LPP_OP_SZ, 0, 0], np.int32)
    args = [C.c_void_p(one[k:].ctypes.data) for k in (0, 1, 1, 1)] + [7, 3, 0] + [None] * 10
    assert _capi.lib().lpp_obs_string_plan_heis(_capi.LPP_STRING_MANY_POINT, 1, *args) == 0
    with pytest.raises(LppError) as ei:
        _capi.check(_capi.lib().lpp_obs_string_plan_heis(_capi.LPP_STRING_MEASURE, 1, *args))
    assert ei.value.status == 1 and "many-point" in str(ei.value)


def test_planner_under_sanitizers(tmp_path):
    """the host planner in a stand-alone program (its own main) built with the address and undefined-behaviour sanitizers: the strings of this file on the
    six sectors against a chain of one-operator plans, what a launch of 1, 8 and 5 of them uploads against their plans, the refusals, (40;3) and a
    16-operator string at 32 sites; the program prints `ok`"""
    src = os.path.join(ROOT, "lanczosplusplus_amd", "host", "test_heis_string_plan.cpp")
    exe = str(tmp_path / "test_heis_string_plan")
    out = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                          "-I" + os.path.join(ROOT, "lanczosplusplus_amd", "csrc"), "-o", exe, src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout
