"""Host side of the observables (no GPU): sector arithmetic, the per-species tables the operator kernel reads, the doSignGf quirk and the
continued-fraction evaluator, against the literal restatement in tests/obs_reference.py."""
import numpy as np
import pytest

import obs_reference as ref
from lanczosplusplus_amd import LppError, continued_fraction, new_parts, operator_plan


@pytest.mark.parametrize("op", ref.OPS)
def test_sector_arithmetic(op):
    """hasNewParts for every operator, both spins, L = 4, every (nup, ndown) in 0..4, refusals included"""
    L = 4
    for spin in (ref.UP, ref.DOWN):
        for nup in range(L + 1):
            for ndown in range(L + 1):
                if op == "n":  # the reference throws
                    with pytest.raises(LppError):
                        new_parts(op, spin, L, nup, ndown)
                    with pytest.raises(RuntimeError):
                        ref.has_new_parts(op, spin, L, nup, ndown)
                    continue
                assert new_parts(op, spin, L, nup, ndown) == ref.has_new_parts(op, spin, L, nup, ndown), (op, spin, nup, ndown)
    assert new_parts("sz", 0, L, 2, 2) is None
    assert new_parts("c", 0, L, 1, 0) is None and new_parts("cdagger", 1, L, 2, 4) is None and new_parts("c", 1, L, 2, 0) is None
    assert new_parts("splus", 0, L, 4, 1) is None and new_parts("sminus", 0, L, 0, 1) is None
    assert new_parts("c", 0, L, 2, 2) == (1, 2) and new_parts("splus", 1, L, 2, 2) == (3, 1)


def _check_tables(op, L, parts):
    for spin in (ref.UP, ref.DOWN):
        want_parts = ref.new_sector(op, spin, L, *parts)
        for site in range(L):
            plan = operator_plan(op, site, spin, L, *parts)
            if want_parts is None:
                assert plan is None
                continue
            assert (plan["nup"], plan["ndown"]) == want_parts
            idx_r, coef_r = ref.action(op, L, parts, want_parts, site, spin)
            idx_t, coef_t = ref.tables_action(plan, op, L, parts)
            assert np.array_equal(idx_t, idx_r), (op, spin, site)  # same destination, same set of non-zero entries
            m = idx_r >= 0
            assert np.array_equal(coef_t[m], coef_r[m]), (op, spin, site)  # same sign / value


@pytest.mark.parametrize("op", ref.OPS)
@pytest.mark.parametrize("L,parts", [(6, (3, 3)), (6, (2, 4)), (6, (6, 1)), (8, (4, 4)), (8, (3, 4)), (8, (4, 3))])
def test_species_tables(op, L, parts):
    _check_tables(op, L, parts)


def test_do_sign_gf_quirk():
    """c, spin down, L = 6: with 3 up electrons site 0 carries the Jordan-Wigner sign and every other site (-1)^3 times it; with 2 up electrons all agree"""
    L = 6
    for parts, factor in (((3, 3), -1.0), ((2, 3), 1.0)):
        new = ref.has_new_parts("c", ref.DOWN, L, *parts)
        for site, f in ((0, 1.0), (2, factor)):
            idx_j, sign_j = ref.jordan_wigner("c", L, parts, new, site, ref.DOWN)
            for idx, coef in (ref.action("c", L, parts, new, site, ref.DOWN), ref.tables_action(operator_plan("c", site, ref.DOWN, L, *parts), "c", L, parts)):
                assert np.array_equal(idx, idx_j)
                m = idx >= 0
                assert m.any() and np.array_equal(coef[m], f * sign_j[m]), (parts, site)
    # spin up has no quirk
    new = ref.has_new_parts("c", ref.UP, L, 3, 3)
    for site in (0, 2):
        idx_j, sign_j = ref.jordan_wigner("c", L, (3, 3), new, site, ref.UP)
        idx, coef = ref.tables_action(operator_plan("c", site, ref.UP, L, 3, 3), "c", L, (3, 3))
        m = idx >= 0
        assert np.array_equal(idx, idx_j) and np.array_equal(coef[m], sign_j[m])


def test_continued_fraction_against_dense_resolvent():
    """G(z) = w [ (z + sigma (T - Eg))^-1 ]_00 for a random 12 x 12 symmetric tridiagonal T"""
    rng = np.random.default_rng(7)
    n = 12
    a = rng.normal(size=n)
    b = np.abs(rng.normal(size=n)) + 0.1  # b[k] couples k and k+1; b[n-1] is the residual the decomposition also returns
    T = np.diag(a) + np.diag(b[:n - 1], 1) + np.diag(b[:n - 1], -1)
    for sigma in (1.0, -1.0):
        rec = dict(a=a, b=b, Eg=-0.7, weight=1.3, sigma=sigma)
        for z in (0.3 + 0.1j, -2.0 + 0.05j, 1.7 + 1.0j, 5.0 + 0.2j, -0.4 + 0.01j):
            M = z * np.eye(n) + sigma * (T - rec["Eg"] * np.eye(n))
            want = rec["weight"] * np.linalg.inv(M)[0, 0]
            got = continued_fraction(rec, z)
            assert abs(got - want) <= 1e-12 * abs(want), (sigma, z, got, want)
    zs = np.array([0.3 + 0.1j, 1.0 + 0.1j])
    both = continued_fraction(rec, zs)
    assert both.shape == (2,) and both[0] == continued_fraction(rec, zs[0])


def test_planners_under_sanitizers(tmp_path):
    """the one-operator planners of the three bases in a stand-alone program (its own main) built with the address and undefined-behaviour sanitizers:
    for every operator, spin and site of small, odd and limiting sectors the expanded plan stays inside the source sector, uses no source twice and
    touches as many destinations as a closed form or a brute-force word list says; the program prints `ok`"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "lanczosplusplus_amd", "host", "test_obs_plan.cpp")
    exe = str(tmp_path / "test_obs_plan")
    out = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "lanczosplusplus_amd", "csrc"), "-o", exe, src],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout
