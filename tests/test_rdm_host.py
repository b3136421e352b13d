"""Host part of the reduced density matrix (no GPU): the planner lpp_rdm_plan against the basis words, and the block form against the literal
restatement of the reference's double loop -- the convention (conjugate on the row index, alpha words) is pinned here before any kernel runs."""
import ctypes as C

import numpy as np
import pytest

import oracle
import rdm_reference as ref
from lanczosplusplus_amd import LppError, _capi, rdm_plan

HUBBARD = [(4, 2, 2, 2), (5, 2, 3, 2), (5, 3, 1, 3), (4, 2, 1, 0), (4, 1, 2, 4), (8, 4, 4, 3), (8, 4, 3, 5)]
SPIN_HALF = [(6, 3, 0, 2), (7, 3, 0, 7)]
CASES = [c + ("hubbard",) for c in HUBBARD] + [c + ("spin_half",) for c in SPIN_HALF]


@pytest.mark.parametrize("L,nup,ndown,split,basis", CASES)
def test_plan_against_the_basis_words(L, nup, ndown, split, basis):
    got = rdm_plan(L, nup, ndown, split, basis)
    want = ref.plan(L, nup, ndown, split, basis)
    assert got["total"] == want["total"] and got["states"] == want["states"]
    assert len(got["blocks"]) == len(want["blocks"])
    for g, w in zip(got["blocks"], want["blocks"]):
        for key in ("k_up", "k_down", "dim_up", "dim_down", "dim", "env_up", "env_down", "terms", "offset"):
            assert g[key] == w[key], (key, g, w)
        assert np.array_equal(g["alpha"], w["alpha"])
        assert np.array_equal(got["starts_up"][g["k_up"]], w["starts_up"])
        assert np.array_equal(got["starts_down"][g["k_down"]], w["starts_down"])
    assert sum(b["dim"] * b["terms"] for b in got["blocks"]) == got["states"]  # V is a re-indexing of psi
    assert got["blocks"] == sorted(got["blocks"], key=lambda b: (b["k_down"], b["k_up"]))
    if split == 0:
        assert [(b["dim"], b["terms"]) for b in got["blocks"]] == [(1, got["states"])]
    if split == L:
        assert [(b["dim"], b["terms"]) for b in got["blocks"]] == [(got["states"], 1)]


def test_sizes_only_call():
    nb, tot, rows = C.c_int32(), C.c_int64(), C.c_int64()
    _capi.check(_capi.lib().lpp_rdm_plan(0, 8, 4, 4, 4, C.byref(nb), C.byref(tot), C.byref(rows), None, None, None, None, None, None))
    assert (nb.value, tot.value, rows.value) == (25, 4900, 256)  # sum_k C(4,k)^2 = 70; sum of d = 4^4


@pytest.mark.parametrize("dtype", ["f64", "c128"])
@pytest.mark.parametrize("L,nup,ndown,split", HUBBARD[:5])
def test_blocks_scattered_equal_the_literal_loop(L, nup, ndown, split, dtype):
    n = oracle.hubbard_basis_words(L, nup, ndown)[0].size
    psi = oracle.fill_random(n, 7, dtype == "c128")
    psi /= np.linalg.norm(psi)
    want = ref.literal(L, nup, ndown, split, psi)
    got = ref.scatter(ref.blocks(L, nup, ndown, split, psi), 4 ** split, psi.dtype)
    assert np.max(np.abs(got - want)) <= 1e-15
    assert abs(np.trace(got) - 1) <= 1e-14
    if dtype == "c128" and 0 < split < L:
        assert np.max(np.abs(want - want.T)) > 1e-3  # the conjugate on the row index is visible: the matrix is not its transpose


@pytest.mark.parametrize("L,nup,ndown,split", SPIN_HALF)
def test_spin_half_blocks_equal_the_literal_loop(L, nup, ndown, split):
    n = len(oracle.heis_basis(L, 1, nup))
    psi = oracle.fill_random(n, 9, True)
    want = ref.literal(L, nup, ndown, split, psi, "spin_half")
    got = ref.scatter(ref.blocks(L, nup, ndown, split, psi, "spin_half"), 2 ** split, psi.dtype)
    assert np.max(np.abs(got - want)) <= 1e-15 * np.max(np.abs(want))


def test_refusals():
    for args in ((4, 2, 2, -1), (4, 2, 2, 5), (4, 5, 2, 2), (4, 2, -1, 2)):
        with pytest.raises(LppError) as ei:
            rdm_plan(*args)
        assert ei.value.status == _capi.LPP_ERR_INVALID
    with pytest.raises(ValueError):
        rdm_plan(4, 2, 2, 2, basis="spin_one")
    with pytest.raises(LppError):
        _capi.check(_capi.lib().lpp_rdm_plan(2, 4, 2, 2, 2, None, None, None, None, None, None, None, None, None))
    assert rdm_plan(6, 3, 99, 2, "spin_half")["states"] == 20  # ndown is ignored for the one-species basis


def test_abi_version():
    assert _capi.LPP_ABI_VERSION == 7 and _capi.lib().lpp_abi_version() == 7
