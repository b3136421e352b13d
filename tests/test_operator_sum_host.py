"""CPU tests of the site-weighted operator sums: the fused plan (lanczosplusplus_amd.operator_sum_plan, csrc/lpp_obs_sum_plan.h) expanded on the host
against sum_r f_r * (the per-site restatement of the reference, tests/obs_reference.py), the linear algebra of the f64 split, the momentum weights, and
the planner in a stand-alone program under the sanitizers."""
import os
import subprocess
from math import comb

import numpy as np
import pytest

import oracle
import operator_sum_reference as sref
import obs_reference as ref
import lanczosplusplus_amd as lp
from lanczosplusplus_amd import geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _weights(L, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(L) + 1j * rng.standard_normal(L)


def _expand(plan, src):
    """z[d] = sum_t factor[d, t] * src[plan.src[d, t]], the terms added in the kernel's order"""
    z = np.zeros(plan["n_dst"], np.complex128)
    for t in range(plan["width"]):
        z = z + plan["factor"][:, t] * src[plan["src"][:, t]]
    return z


@pytest.mark.parametrize("L,nup,ndown", sref.HOST_SECTORS)
@pytest.mark.parametrize("op", sref.FUSED_OPS)
@pytest.mark.parametrize("spin", (ref.UP, ref.DOWN))
def test_plan_expanded_equals_the_site_loop(op, spin, L, nup, ndown):
    f = _weights(L, 7 * L + nup)
    n_src = comb(L, nup) * comb(L, ndown)
    src = oracle.fill_random(n_src, 31) + 1j * oracle.fill_random(n_src, 32)
    want, new = sref.hubbard_sum(op, spin, L, (nup, ndown), f, src)
    plan = lp.operator_sum_plan(op, spin, L, nup, ndown, f)
    if want is None:
        assert plan is None
        return
    assert (plan["nup"], plan["ndown"]) == new and plan["n_dst"] == len(want)
    W = sref.width(op, spin, L, new)
    assert plan["width"] == W and plan["src"].shape == (len(want), W)
    assert np.all((plan["src"] >= 0) & (plan["src"] < n_src))
    if op in ("c", "cdagger"):
        assert np.all(np.diff(plan["site"], axis=1) > 0) and plan["site"].min() >= 0 and plan["site"].max() < L  # ascending site
        signs = lp.operator_sum_plan(op, spin, L, nup, ndown)["factor"]  # unit weights: the factor is the sign
        assert np.all(np.abs(signs) == 1.0) and np.all(signs.imag == 0.0)
    got = _expand(plan, src)
    assert np.max(np.abs(got - want)) <= sref.bound(W, f, src)


def test_no_sector_and_refusals():
    assert lp.operator_sum_plan("cdagger", ref.UP, 6, 6, 3) is None  # a full up species
    assert lp.operator_sum_plan("c", ref.DOWN, 6, 3, 0) is None
    assert lp.operator_sum_plan("c", ref.UP, 6, 1, 0) is None  # the (0, 0) sector
    assert lp.operator_sum_plan("cdagger", ref.DOWN, 6, 3, 6) is None
    for op in ("splus", "sminus"):
        with pytest.raises(lp.LppError):
            lp.operator_sum_plan(op, ref.UP, 6, 3, 3)
    for bad in ((31, 3, 3), (6, 7, 3), (6, 3, -1), (0, 0, 0)):
        with pytest.raises((lp.LppError, ValueError)):
            lp.operator_sum_plan("c", ref.UP, *bad)
    with pytest.raises(lp.LppError):
        lp.operator_sum_plan("c", 2, 6, 3, 3)
    with pytest.raises(ValueError):
        lp.operator_sum_plan("c", ref.UP, 6, 3, 3, np.ones(5))


def test_momentum_weights():
    L = 6
    for m in range(L):
        w = geometry.momentum_weights(np.arange(L), 2 * np.pi * m / L)
        # the two sides round the phase q x (up to 2 pi (L - 1)) differently: a few ulps of the phase is the error of the exponential
        assert np.max(np.abs(w - sref.momentum_weights(L, m))) <= 4 * 2.2e-16 * 2 * np.pi * (L - 1)
    # commensurate phases are exact: sin(pi r) = 1.2e-16 r would pass for a weight, launch a site in the chain and get a record in the f64 split
    for L in (6, 8, 16):
        pos = np.arange(L)
        assert np.all(geometry.momentum_weights(pos, np.pi).imag == 0) and np.all(geometry.momentum_weights(pos, 0.0).imag == 0)
        assert np.array_equal(geometry.momentum_weights(pos, np.pi) * np.sqrt(L), (-1.0) ** pos + 0j)
        quarter = geometry.momentum_weights(pos, np.pi / 2)
        assert np.all(quarter.real[1::2] == 0) and np.all(quarter.imag[0::2] == 0)
    sq = geometry.momentum_weights([[x, y] for x in range(4) for y in range(4)], [np.pi / 2, np.pi / 2])
    assert np.count_nonzero(sq.real) == 8 and np.count_nonzero(sq.imag) == 8
    w2 = geometry.momentum_weights([[0, 0], [1, 0], [0, 1], [1, 1]], [np.pi, np.pi / 2])
    assert np.max(np.abs(w2 - 0.5 * np.array([1, -1, 1j, -1j]))) <= 1e-15
    with pytest.raises(ValueError):
        geometry.momentum_weights(np.arange(4), [1.0, 2.0])


def test_f64_split_is_exact_linear_algebra():
    """H real symmetric, gs real, |phi> = C + i S with real C, S: <phi|G(z)|phi> = G_CC + G_SS, the cross terms cancel.  6-site ring, (3, 3),
    c up with complex weights; dense (z - (H - Eg))^-1 from oracle.hubbard_csr; 1e-12 relative."""
    L, parts = 6, (3, 3)
    hop = np.zeros((L, L))
    for i in range(L):
        hop[i, (i + 1) % L] = hop[(i + 1) % L, i] = -1.0
    U = np.full(L, 4.0)

    def dense(p):
        A = oracle.hubbard_csr(L, p[0], p[1], hop, U)
        n = A.nrows
        H = np.zeros((n, n))
        for i in range(n):
            H[i, A.colind[A.rowptr[i]:A.rowptr[i + 1]]] = np.real(A.values[A.rowptr[i]:A.rowptr[i + 1]])
        return H

    w0, v0 = np.linalg.eigh(dense(parts))
    eg, gs = w0[0], v0[:, 0]
    f = _weights(L, 5)
    phi, new = sref.hubbard_sum("c", ref.UP, L, parts, f, gs)
    Cv, _ = sref.hubbard_sum("c", ref.UP, L, parts, f.real, gs)
    Sv, _ = sref.hubbard_sum("c", ref.UP, L, parts, f.imag, gs)
    assert new == (2, 3) and np.isrealobj(Cv) and np.isrealobj(Sv)
    H2 = dense(new)
    z = np.linspace(-6.0, 6.0, 13) + 0.1j
    whole = sref.dense_resolvent(H2, eg, phi, z)
    parts_sum = sref.dense_resolvent(H2, eg, Cv, z) + sref.dense_resolvent(H2, eg, Sv, z)
    assert np.max(np.abs(whole - parts_sum)) <= 1e-12 * np.max(np.abs(whole))
    assert abs(np.vdot(phi, phi).real - (Cv @ Cv + Sv @ Sv)) <= 1e-12 * np.vdot(phi, phi).real


def test_sum_planner_under_sanitizers(tmp_path):
    """host/test_obs_sum_plan.cpp (its own main, the plan headers alone) built with the address and undefined-behaviour sanitizers: every sector with
    L <= 7 has exactly W entries per destination, no rank out of range, the refusals of obs_plan; the program prints `ok`"""
    src = os.path.join(ROOT, "lanczosplusplus_amd", "host", "test_obs_sum_plan.cpp")
    exe = str(tmp_path / "test_obs_sum_plan")
    out = subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "lanczosplusplus_amd", "csrc"), "-o", exe, src],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout
