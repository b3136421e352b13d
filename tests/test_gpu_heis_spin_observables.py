"""Spin-S Heisenberg observables on the GPU (the opt-in digit basis, basis="spin"): operator application in the BasisHeisenberg digit order, two-point
correlations, spectral functions, site-weighted sums and the lanczos driver, against the literal restatement in tests/heis_spin_obs_reference.py (word
list by recursion + dictionary search, no runs) and the oracle's matrices of the sectors.  Tolerances are those of tests/test_gpu_heis_observables.py
and, for the chained sums, of tests/test_gpu_operator_sum.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import heis_spin_obs_reference as ref
import operator_sum_reference as sref
import oracle
from helpers import chain, rel
from lanczosplusplus_amd import LanczosEngine, LppError, continued_fraction, geometry, operator_plan_heis_spin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "lanczosplusplus_amd", "host", "lanczos")
GOLD = os.path.join(ROOT, "tests", "golden")
NAME = "heisenberg_spin1_L8_obs.inp"
PLAIN = "heisenberg_spin1_L8.inp"

pytestmark = pytest.mark.gpu


def _golden_model(name=NAME):
    """(L, twiceS, szPlusConst, jpm, jzz, field, anisotropy) of the golden S = 1 ring: 8 sites, szPlusConst = 8 (Sz = 0), 1107 states"""
    inp = geometry.parse_input(open(os.path.join(GOLD, name)).read())
    assert inp["Model"] == "Heisenberg"
    terms = geometry.terms_from_input(inp)
    return (int(inp["TotalNumberOfSites"]), int(inp["HeisenbergTwiceS"]), int(inp["TargetSzPlusConst"]), terms[0], terms[1],
            np.asarray(inp["MagneticField"], np.float64), np.asarray(inp["AnisotropyD"], np.float64))


def test_the_fixture_is_the_plain_input_with_the_token():
    a = open(os.path.join(GOLD, PLAIN)).read().splitlines()
    b = open(os.path.join(GOLD, NAME)).read().splitlines()
    assert len(a) == len(b) and [(x, y) for x, y in zip(a, b) if x != y] == [("SolverOptions=none", "SolverOptions=HeisenbergSpinObservables")]


# ---- 1. operator application ------------------------------------------------------------------------------------------------------------------
# (5;2;4): 45 states, the f64 half-unit tail, one run.  (11;2;11): 25653 states, odd, 13 tiles of 1024 units in f64, 243 runs of 1 .. 141 elements, five
# sites above the cut at lb = 6.  (7;4;13): 3-bit digits whose codes 5-7 never occur, lb = 4.  (24;2;3): 18 high digits, most runs hold a few elements.
STATES = {(5, 2, 4): 45, (11, 2, 11): 25653, (7, 4, 13): 7875, (24, 2, 3): 2576}


@pytest.mark.parametrize("dtype", ["f64", "c128"])
@pytest.mark.parametrize("sector", sorted(STATES))
def test_apply_operator_heis_spin(dtype, sector):
    """sz, splus, sminus at site 0, the last site below the cut, the first at or above it and L-1: each output element is one product"""
    L, t, m = sector
    cplx = dtype == "c128"
    n = ref.size(L, t, m)
    assert n == STATES[sector]
    src = oracle.fill_random(n, 11, cplx)
    factor = (0.75 - 0.5j) if cplx else -1.25
    lb = operator_plan_heis_spin("sz", 0, L, t, m)["lb"]
    assert lb == {2: min(L, 6), 4: 4}[t]
    sites = sorted({0, lb - 1, min(lb, L - 1), L - 1})
    assert (L <= lb) or (any(s < lb for s in sites) and any(s >= lb for s in sites))
    with LanczosEngine(dtype=dtype) as e:
        for op in ref.OPS:
            new = ref.new_sector(op, L, t, m)
            for site in sites:
                z, got_parts = e.apply_operator(op, site, 0, L, m, 0, src, factor=factor, basis="spin", twiceS=t)
                assert got_parts == (new, 0) and len(z) == ref.size(L, t, new)
                want = ref.apply(np.zeros(len(z), src.dtype), op, L, t, m, src, site, factor)
                assert np.max(np.abs(want)) > 0
                assert np.max(np.abs(z - want)) <= 1e-14 * np.max(np.abs(want)), (op, site)
                untouched = ~ref.touched(op, L, t, m, site)
                assert untouched.any() and np.all(z[untouched] == 0), (op, site)  # (S = 1, 2: m = 0 is a digit, so sz leaves destinations out too)
                # z += ...: a second application on top of the first
                z2, _ = e.apply_operator(op, site, 1, L, m, 0, src, factor=factor, out=z, basis="spin", twiceS=t)  # (the spin is not read)
                assert np.max(np.abs(z2 - 2 * want)) <= 2e-14 * np.max(np.abs(want)) and np.all(z2[untouched] == 0)
        # the other kind of factor: a real one on c128; a complex one on an f64 engine is refused
        want = ref.apply(np.zeros(ref.size(L, t, m + 1), src.dtype), "splus", L, t, m, src, sites[-1], -1.25)
        if cplx:
            z, _ = e.apply_operator("splus", sites[-1], 0, L, m, 0, src, factor=-1.25, basis="spin", twiceS=t)
            assert np.max(np.abs(z - want)) <= 1e-14 * np.max(np.abs(want))
        else:
            with pytest.raises(LppError) as ei:
                e.apply_operator("splus", sites[-1], 0, L, m, 0, src, factor=0.75 - 0.5j, basis="spin", twiceS=t)
            assert ei.value.status == 1
        # refusals are status codes, never a launch
        for op in ("n", "c", "cdagger"):
            with pytest.raises(LppError) as ei:
                e.apply_operator(op, 0, 0, L, m, 0, src, basis="spin", twiceS=t)
            assert ei.value.status == 1
        with pytest.raises(LppError) as ei:
            e.apply_operator("sminus", 0, 0, L, 0, 0, np.ones(1, src.dtype), basis="spin", twiceS=t)
        assert ei.value.status == 1
        with pytest.raises(LppError) as ei:
            e.apply_operator("splus", 0, 0, L, L * t, 0, np.ones(1, src.dtype), basis="spin", twiceS=t)
        assert ei.value.status == 1
        with pytest.raises(LppError) as ei:
            e.apply_operator("sz", 0, 0, L, m, 0, src, basis="spin", twiceS=5)  # a spin the assembler refuses
        assert ei.value.status == 1
        with pytest.raises(ValueError):
            e.apply_operator("sz", 0, 0, L, m, 0, src, basis="spin")  # twiceS is required
        with pytest.raises(ValueError):
            e.apply_operator("sz", 0, 0, L, m, 0, src, basis="heisenberg")


def test_twice_s_one_equals_the_spin_half_kernel():
    """(16;1;7), 11440 states, one-bit digits cut at 12: splus / sminus through the digit-basis kernel equal basis="spin_half" bit for bit, sz equals
    -1/2 times the raw 1 - 2 bit bit for bit"""
    L, m = 16, 7
    src = oracle.fill_random(11440, 3)
    with LanczosEngine() as e:
        for site in (0, 11, 12, 15):
            for op in ("splus", "sminus", "sz"):
                a, pa = e.apply_operator(op, site, 0, L, m, 0, src, factor=-1.25, basis="spin_half")
                b, pb = e.apply_operator(op, site, 0, L, m, 0, src, factor=-1.25, basis="spin", twiceS=1)
                assert pa == pb and np.any(a != 0)
                want = -0.5 * a if op == "sz" else a
                assert np.array_equal(b.view(np.uint64), want.view(np.uint64)), (op, site)


# ---- 2. two-point correlations ------------------------------------------------------------------------------------------------------------------
def test_two_point_heis_spin():
    """<S^z_j S^z_i> and <S^-_j S^+_i> on the golden S = 1 ring with its field and anisotropy, the sum rules, bra != ket, and the refusal without the
    opt-in"""
    L, t, m, jpm, jzz, h, d = _golden_model()
    assert (L, t, m) == (8, 2, 8) and ref.size(L, t, m) == 1107
    S = t / 2
    with LanczosEngine(reortho=True, max_steps=150, eps=1e-11) as e:
        e.assemble_heisenberg(L, m, jpm, jzz, h, twiceS=t, anisotropy=d)
        e.keep_states(2)
        e.lanczos(2, want_vectors=False)
        gs, ex = e.state(0), e.state(1)
        got = {}
        for op in ("sz", "splus"):
            res, tr = e.two_point(op, basis="spin")
            want, wtr = ref.two_point(op, L, t, m, gs, gs)
            scale = np.max(np.abs(want))
            print("two_point spin-1 %s: max deviation %.3e of %.3e" % (op, np.max(np.abs(res - want)), scale))
            assert np.max(np.abs(res - want)) <= 1e-12 * scale, op
            assert abs(tr - np.trace(res)) <= 1e-12 * scale and abs(tr - wtr) <= 1e-11 * scale
            got[op] = (res, tr)
        # sum_ij <S^z_i S^z_j> = (total S^z)^2 = (szPlusConst - L S)^2
        assert abs(np.sum(got["sz"][0]) - (m - L * S) ** 2) <= 1e-10
        # S^- S^+ = S(S+1) - m^2 - m per site; sum_i <m_i^2> is the trace of the sz matrix, sum_i <m_i> = szPlusConst - L S
        assert abs(got["splus"][1] - (L * S * (S + 1) - got["sz"][1] - (m - L * S))) <= 1e-10
        # <bra| ... |ket> between two resident states: absolute, as the two states are orthogonal; each entry is a dot product of two vectors of norm
        # <= S(S+1) = 2 over 1107 terms, whose rounding error is far below 1107 * 1.1e-16 * 2 = 2.5e-13
        for op in ("sz", "splus"):
            res, tr = e.two_point(op, bra=1, ket=0, basis="spin")
            want, wtr = ref.two_point(op, L, t, m, ex, gs)
            assert np.max(np.abs(want)) > 1e-6 and np.max(np.abs(res - want)) <= 1e-12, op
            assert abs(tr - wtr) <= 1e-11
        # without the opt-in the same engine answers as before
        for call in (lambda: e.two_point("sz"), lambda: e.spectral_function("sz", 0, 0), lambda: e.weighted_norm2("sz", np.ones(L))):
            with pytest.raises(LppError) as ei:
                call()
            assert ei.value.status == 1
        for op in ("n", "c"):
            with pytest.raises(LppError) as ei:
                e.two_point(op, basis="spin")
            assert ei.value.status == 1
        with pytest.raises(ValueError):
            e.two_point("sz", basis="heisenberg")
        assert e.sector_assemblies == 0
    with LanczosEngine() as e:  # an engine that is not a Heisenberg one
        hop = chain(4, -1.0, True)
        e.assemble_hubbard(4, 2, 2, hop, np.full(4, 4.0))
        e.keep_states(1)
        e.lanczos(1, want_vectors=False)
        with pytest.raises(LppError) as ei:
            e.two_point("sz", basis="spin")
        assert ei.value.status == 1


def test_energy_identity_of_the_isotropic_ring():
    """isotropic S = 1 ring of 6 sites, jpm = jzz = 1, no field, Sz = 0 (141 states): the ground state is a singlet, so E0 = sum over the L bonds of
    <S.S> = 3 L <S^z_0 S^z_1>.  -8.617423181814 on both sides (checked with numpy).  The identity is linear in the error of the STATE, which an
    energy criterion does not see (its error is quadratic), so eps = 0 switches the criterion off: the recurrence runs with reorthogonalisation
    until the Krylov space is exhausted, 141 steps at the most, and the Ritz vector is converged to rounding."""
    L, t, m = 6, 2, 6
    assert ref.size(L, t, m) == 141
    with LanczosEngine(reortho=True, max_steps=141, eps=0.0) as e:
        e.assemble_heisenberg(L, m, chain(L, 1.0, True), chain(L, 1.0, True), twiceS=t)
        e.keep_states(1)
        eg, _, _ = e.lanczos(1, want_vectors=False)
        res, _ = e.two_point("sz", basis="spin")
        print("energy identity: E0 %.12f, 3 L <Sz0 Sz1> %.12f" % (eg[0], 3 * L * res[0, 1]))
        assert abs(eg[0] - (-8.617423181814)) <= 1e-10
        assert abs(eg[0] - 3 * L * res[0, 1]) <= 1e-10


# ---- 3. spectral function -----------------------------------------------------------------------------------------------------------------------
_DENSE = {}


def _dense_sector(key, A):
    if key not in _DENSE:
        _DENSE[key] = np.linalg.eigh(A.to_scipy().toarray())
    return _DENSE[key]


def _lehmann(w_eig, v_eig, modif, ws2, sigma, eg, z):
    ov = np.abs(v_eig.conj().T @ modif) ** 2
    wn = np.vdot(modif, modif).real
    return (ws2 / wn) * np.sum(ov[None, :] / (z[:, None] + sigma * (w_eig[None, :] - eg)), axis=1)


def test_spectral_function_heis_spin():
    """sz and splus on the golden S = 1 model: types, sectors, sigma and weights as the restatement, a / b against the oracle's decomposition of the
    restatement's modified vector on the oracle's matrix of the new sector (1016, 1107 and 1016 states), the Lehmann sum from the dense spectrum of
    that sector, the resident state unchanged, three sector assemblies"""
    L, t, m, jpm, jzz, field, d = _golden_model()
    omega = np.arange(-8.0, 8.0 + 1e-9, 0.25) + 0.1j
    with LanczosEngine() as e:
        e.assemble_heisenberg(L, m, jpm, jzz, field, twiceS=t, anisotropy=d)
        e.keep_states(1)
        eg, _, _ = e.lanczos(1, want_vectors=False)
        gs = e.state(0)
        before = gs.copy()
        for op in ("sz", "splus"):
            for (i, j) in ((0, 0), (0, 3), (2, 5)):
                recs = e.spectral_function(op, i, j, basis="spin")
                want = ref.spectral_types(op, L, t, m, gs, i, j)
                assert [r["type"] for r in recs] == [w[0] for w in want] and len(recs) == (2 if i == j else 4)
                for r, (typ, o, new, modif, ws2, msign) in zip(recs, want):
                    assert r["sector"] == (new, 0) and r["sigma"] == msign and r["Eg"] == eg[0]
                    assert new == {"sz": 8, "splus": 9, "sminus": 7}[o]
                    assert abs(r["weight"] - ws2) <= 1e-12 * abs(ws2), (op, i, j, typ, r["weight"], ws2)
                    A = oracle.heis_csr(L, t, new, jpm, jzz, field, aniso=d)
                    assert A.nrows == ref.size(L, t, new) and A.nrows in (1016, 1107)
                    steps, ao, bo, _, _ = oracle.lanczos_decomposition(A, modif)
                    assert r["steps"] == steps and rel(r["a"], ao) < 1e-8 and rel(r["b"], bo) < 1e-8, (op, i, j, typ)
                    w_eig, v_eig = _dense_sector(new, A)
                    exact = _lehmann(w_eig, v_eig, modif, ws2, msign, eg[0], omega)
                    g_gpu = continued_fraction(r, omega)
                    g_orc = continued_fraction(dict(a=ao, b=bo, Eg=eg[0], weight=ws2, sigma=msign), omega)
                    scale = np.max(np.abs(exact))
                    d_orc, d_gpu = np.max(np.abs(g_orc - exact)) / scale, np.max(np.abs(g_gpu - exact)) / scale
                    print("lehmann spin-1 %s pair (%d,%d) type %d: oracle %.3e gpu %.3e" % (op, i, j, typ, d_orc, d_gpu))
                    # ten times what the oracle's own decomposition of the same vector deviates from the Lehmann sum by (test_spectral_function_heis)
                    assert d_gpu <= 10 * d_orc, (op, i, j, typ, d_gpu, d_orc)
        assert e.sector_assemblies == 3 and sorted(e._sectors) == [(7, 0), (8, 0), (9, 0)]  # the engine's own sector has an engine of its own
        assert np.array_equal(e.state(0).view(np.uint64), before.view(np.uint64))
        with pytest.raises(LppError) as ei:
            e.spectral_function("n", 0, 0, basis="spin")
        assert ei.value.status == 1 and e.sector_assemblies == 3


# ---- 4. site-weighted sums ------------------------------------------------------------------------------------------------------------------------
def _sum_reference(op, L, t, m, f, src):
    z = np.zeros(ref.size(L, t, ref.new_sector(op, L, t, m)), np.result_type(src.dtype, np.asarray(f).dtype))
    for r in range(L):
        ref.apply(z, op, L, t, m, src, r, f[r])
    return z


@pytest.mark.parametrize("dtype", ["f64", "c128"])
def test_operator_sums_heis_spin(dtype):
    """apply_operator_sum (the chain of one-site launches) and weighted_norm2 against sum_r f_r A_r of the restatement, to the bound
    tests/test_gpu_operator_sum.py has for chained families: 4 (L + 2) eps sum|f| max|src| per element"""
    L, t, m = 9, 2, 8  # 2907 states, three sites above the cut
    cplx = dtype == "c128"
    rng = np.random.default_rng(5)
    f = rng.standard_normal(L) + (1j * rng.standard_normal(L) if cplx else 0)
    f[3] = 0  # a site without a weight launches nothing
    src = oracle.fill_random(ref.size(L, t, m), 23, cplx)
    tol = sref.bound(L, f, src)
    with LanczosEngine(dtype=dtype) as e:
        for op in ref.OPS:
            z, new = e.apply_operator_sum(op, 0, f, L, m, 0, src, basis="spin", twiceS=t)
            want = _sum_reference(op, L, t, m, f, src)
            assert new == (ref.new_sector(op, L, t, m), 0) and len(z) == len(want)
            assert np.max(np.abs(z - want)) <= tol, (op, np.max(np.abs(z - want)), tol)
            z2, _ = e.apply_operator_sum(op, 0, f, L, m, 0, src, out=z.copy(), basis="spin", twiceS=t)
            assert np.max(np.abs(z2 - 2 * want)) <= 2 * tol, op
        zero, _ = e.apply_operator_sum("sz", 0, np.zeros(L), L, m, 0, src, basis="spin", twiceS=t)
        assert not zero.any()
        with pytest.raises(LppError) as ei:
            e.apply_operator_sum("n", 0, f, L, m, 0, src, basis="spin", twiceS=t)
        assert ei.value.status == 1


def test_weighted_norm2_and_spectral_function_k_heis_spin():
    """the static structure factor <phi|phi> of S^z_q and S^+_q on the golden model against the restatement, and one S^zz(q = pi, w) record against
    the oracle's decomposition of the restatement's vector"""
    L, t, m, jpm, jzz, field, d = _golden_model()
    pos = np.arange(L)
    with LanczosEngine() as e:
        e.assemble_heisenberg(L, m, jpm, jzz, field, twiceS=t, anisotropy=d)
        e.keep_states(1)
        eg, _, _ = e.lanczos(1, want_vectors=False)
        gs = e.state(0)
        for op in ("sz", "splus"):
            for q in (0.0, np.pi):
                f = geometry.momentum_weights(pos, q).real
                want = _sum_reference(op, L, t, m, f, gs)
                got = e.weighted_norm2(op, f, basis="spin")
                # <phi|phi> of a vector whose elements carry the chained bound: 2 |phi| sqrt(n) bound, and the rounding of the dot product itself
                tol = 2 * np.linalg.norm(want) * np.sqrt(len(want)) * sref.bound(L, f, gs) + 1e-13 * (want @ want)
                assert abs(got - want @ want) <= tol, (op, q, got, want @ want)
        assert abs(e.weighted_norm2("sz", geometry.momentum_weights(pos, 0.0), basis="spin") - (m - L * t / 2) ** 2 / L) <= 1e-10
        recs = e.spectral_function_k("sz", np.pi, pos, basis="spin")
        assert [r["type"] for r in recs] == [0, 1] and all(r["part"] is None and r["sector"] == (m, 0) for r in recs)
        state = _sum_reference("sz", L, t, m, geometry.momentum_weights(pos, np.pi).real, gs)
        steps, ao, bo, _, _ = oracle.lanczos_decomposition(oracle.heis_csr(L, t, m, jpm, jzz, field, aniso=d), state)
        for r in recs:
            s = -1 if r["type"] else 1
            assert r["sigma"] == float(-s) and abs(r["weight"] - s * (state @ state)) <= 1e-12 * (state @ state)
            assert r["steps"] == steps and rel(r["a"], ao) < 1e-8 and rel(r["b"], bo) < 1e-8
        assert e.sector_assemblies == 1
        with pytest.raises(LppError) as ei:
            e.spectral_function_k("sz", np.pi, pos)  # without the opt-in
        assert ei.value.status == 1


# ---- 5. the lanczos driver: -c, -g on an input with the SolverOptions token -------------------------------------------------------------------------
def _python_engine():
    """the Python path on the model of the input file, started from the vector the C++ shim starts from (fillRandom, seed 1234)"""
    L, t, m, jpm, jzz, field, d = _golden_model()
    e = LanczosEngine()
    e.assemble_heisenberg(L, m, jpm, jzz, field, twiceS=t, anisotropy=d)
    e.keep_states(1)
    e.lanczos(1, init=oracle.fill_random(e.rows(), 1234), want_vectors=False)
    return e, L


@pytest.mark.parametrize("op", ["sz", "splus"])
def test_driver_two_point_heis_spin(op):
    """lanczos -f tests/golden/heisenberg_spin1_L8_obs.inp -c <op>: the matrix and the MatrixDiagonal line against two_point of the Python path"""
    assert os.path.exists(DRIVER), "run __graft_entry__.build()"
    res = subprocess.run([DRIVER, "-f", os.path.join(GOLD, NAME), "-c", op, "-p", "14"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    k = next(i for i, ln in enumerate(lines) if ln.startswith("MatrixDiagonal = "))
    assert lines[k - 2] == "spins=0 0" and lines[k - 1] == "orbs=0 0"
    diag = float(lines[k].split("=", 1)[1].strip())
    e, L = _python_engine()
    with e:
        want, wtr = e.two_point(op, basis="spin")
    assert lines[k + 1].split() == [str(L), str(L)]
    got = np.array([[float(x) for x in lines[k + 2 + i].split()] for i in range(L)])
    assert got.shape == (L, L)
    scale = np.max(np.abs(want))
    print("driver spin-1 -c %s: max deviation %.3e of %.3e, MatrixDiagonal %s against %s" % (op, np.max(np.abs(got - want)), scale, diag, wtr))
    assert np.max(np.abs(got - want)) <= 1e-8 * scale
    assert abs(diag - wtr) <= 1e-8


def test_driver_without_the_token_still_refuses():
    """the unchanged heisenberg_spin1_L8.inp with -c sz fails as before: the observables of this model need the opt-in"""
    assert os.path.exists(DRIVER), "run __graft_entry__.build()"
    res = subprocess.run([DRIVER, "-f", os.path.join(GOLD, PLAIN), "-c", "sz"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "twoPoint" in res.stderr and "MatrixDiagonal" not in res.stdout


@pytest.mark.parametrize("args, sentence", [
    (["-M", "sz?0?0;sz?1?0"], "LPP_ERR_INVALID: manyPoint: operator strings are not built for the spin-S digit basis (HeisenbergSpinObservables)"),
    (["-r", "4"], "reducedDensityMatrix: needs a Model of the HubbardOneOrbital family solved by the GPU Lanczos (no symmetry sectors, no dense fallback)")])
def test_driver_with_the_token_refuses_strings_and_the_density_matrix(args, sentence):
    """the two refusals of the shim that name no other model's input: operator strings and -r on the input that opts into the digit basis"""
    assert os.path.exists(DRIVER), "run __graft_entry__.build()"
    res = subprocess.run([DRIVER, "-f", os.path.join(GOLD, NAME)] + args, capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and sentence in res.stderr, res.stderr


def _parse_comb(text):
    """the record layout of INTEGRATION.md"""
    head = dict(re.findall(r"^(Site0|Site1|TSPCenter)=(\d+)$", text, re.M))
    labels = re.search(r"^#INDEXTOCF (.*)$", text, re.M).group(1).split()
    recs = []
    for block in re.split(r"^#ContinuedFraction=\d+\n", text, flags=re.M)[1:]:
        vec = {}
        for key in ("Avector", "Bvector"):
            toks = re.search(r"^#%s (.*)$" % key, block, re.M).group(1).split()
            assert int(toks[0]) == len(toks) - 1
            vec[key] = np.array([float(x) for x in toks[1:]])
        sc = {k: float(v) for k, v in re.findall(r"^#CF(Energy|Weight|Isign)=(\S+)$", block, re.M)}
        recs.append(dict(a=vec["Avector"], b=vec["Bvector"], Eg=sc["Energy"], weight=sc["Weight"], sigma=sc["Isign"]))
    assert len(recs) == len(labels)
    return head, labels, recs


def test_driver_spectral_function_heis_spin(tmp_path):
    """lanczos -g sz with `TSPSites 2 0 3` and SpectralSteps=40 appended to a copy of the input writes <input basename>0.comb; its records against
    spectral_function(basis="spin") of the Python path"""
    assert os.path.exists(DRIVER), "run __graft_entry__.build()"
    inp = tmp_path / "heis.inp"
    inp.write_text(open(os.path.join(GOLD, NAME)).read().rstrip("\n") + "\nTSPSites 2 0 3\nSpectralSteps=40\n")
    res = subprocess.run([DRIVER, "-f", str(inp), "-g", "sz", "-p", "14"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr
    assert "#gf(i=0, j=3)" in res.stdout.splitlines()
    assert "#SectorAssemblies=1" in res.stderr
    comb = tmp_path / "heis.inp0.comb"
    assert comb.exists(), os.listdir(str(tmp_path))
    head, labels, recs = _parse_comb(comb.read_text())
    assert head == {"Site0": "0", "Site1": "3"} and labels == ["0,0,0,0", "0,1,0,0", "0,2,0,0", "0,3,0,0"]
    e, L = _python_engine()
    with e:
        want = e.spectral_function("sz", 0, 3, 0, max_steps=40, basis="spin")
        assert [w["label"] for w in want] == labels and {w["sector"] for w in want} == {(8, 0)}
        for r, w in zip(recs, want):
            print("driver spin-1 -g sz type %d: steps %d / %d" % (w["type"], len(r["a"]), w["steps"]))
            assert len(r["a"]) == len(r["b"]) == w["steps"] <= 40
            assert rel(r["a"], w["a"]) < 1e-8 and rel(r["b"], w["b"]) < 1e-8
            assert abs(r["weight"] - w["weight"]) <= 1e-8 * abs(w["weight"]) and r["sigma"] == w["sigma"]
            assert abs(r["Eg"] - w["Eg"]) <= 1e-8 * abs(w["Eg"])
            z = np.array([-1.0 + 0.1j, 0.5 + 0.1j, 2.0 + 0.1j])
            assert np.max(np.abs(continued_fraction(r, z) - continued_fraction(w, z))) <= 1e-8 * np.max(np.abs(continued_fraction(w, z)))
