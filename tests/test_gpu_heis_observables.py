"""S = 1/2 Heisenberg observables on the GPU: operator application in the BasisHeisenberg order, resident states of the chain form, two-point
correlations and spectral functions, against the literal restatement of the reference in tests/heis_obs_reference.py (word list + search, no runs).
Tolerances are those of tests/test_gpu_tj_observables.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import heis_obs_reference as ref
import oracle
from helpers import chain, rel
from lanczosplusplus_amd import LanczosEngine, LppError, continued_fraction, geometry, operator_plan_heis
from lanczosplusplus_amd._capi import Stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "lanczosplusplus_amd", "host", "lanczos")
GOLD = os.path.join(ROOT, "tests", "golden")
NAME = "heisenberg_chain_L12.inp"

pytestmark = pytest.mark.gpu


def _golden_model(name=NAME):
    inp = geometry.parse_input(open(os.path.join(GOLD, name)).read())
    assert inp["Model"] == "Heisenberg" and int(inp["HeisenbergTwiceS"]) == 1
    terms = geometry.terms_from_input(inp)
    return int(inp["TotalNumberOfSites"]), int(inp["TargetSzPlusConst"]), terms[0], terms[1], np.asarray(inp["MagneticField"], np.float64)


def _force_chain(monkeypatch, on):
    """the chain form (layout kernel 4) below the size from which it is chosen by itself, as tests/test_gpu_parity.py forces it"""
    monkeypatch.setenv("LPP_PRODUCT_LAYOUT", "1" if on else "0")
    monkeypatch.setenv("LPP_PB_PIECE_ROWS", "256")


# ---- 1. operator application ------------------------------------------------------------------------------------------------------------------
# (7;2) -> (7;3): 21 -> 35 states, the f64 half-unit tail, one run (no site above the cut).  (16;7): 11440 -> 12870 or 8008 states, several tiles of
# 1024 units, 16 high parts.  (18;9): 48620 states in 64 runs of 1 .. 924 elements; the cut of the word is at 12 bits, so L = 16 and 18 have sites
# on both sides of it.
@pytest.mark.parametrize("dtype", ["f64", "c128"])
@pytest.mark.parametrize("L,m", [(7, 2), (16, 7), (18, 9)])
def test_apply_operator_heis(dtype, L, m):
    """every operator and spin at site 0, the last site below the cut, the first at or above it and L-1: each output element is one product"""
    cplx = dtype == "c128"
    n = ref.size(L, m)
    assert n == {7: 21, 16: 11440, 18: 48620}[L]
    src = oracle.fill_random(n, 11, cplx)
    factor = (0.75 - 0.5j) if cplx else -1.25
    lb = operator_plan_heis("sz", 0, ref.UP, L, m)["lb"]
    assert lb == min(L, 12)
    sites = sorted({0, lb - 1, min(lb, L - 1), L - 1})
    assert (L <= 12) or (any(s < lb for s in sites) and any(s >= lb for s in sites))
    sizes = set()
    with LanczosEngine(dtype=dtype) as e:
        for op in ref.OPS:
            for spin in (ref.UP, ref.DOWN):
                new = ref.new_sector(op, spin, L, m)
                for site in sites:
                    z, got_parts = e.apply_operator(op, site, spin, L, m, 0, src, factor=factor, basis="spin_half")
                    assert got_parts == (new, 0) and len(z) == ref.size(L, new)
                    sizes.add(len(z))
                    want = ref.acc_modified_state_(np.zeros(len(z), src.dtype), op, L, m, new, src, site, spin, factor)
                    assert np.max(np.abs(want)) > 0
                    assert np.max(np.abs(z - want)) <= 1e-14 * np.max(np.abs(want)), (op, spin, site)
                    untouched = ~ref.touched(op, L, m, new, site, spin)
                    assert (op == "sz") == (not untouched.any()) and np.all(z[untouched] == 0), (op, spin, site)
                    # z += ...: a second application on top of the first
                    z2, _ = e.apply_operator(op, site, spin, L, m, 0, src, factor=factor, out=z, basis="spin_half")
                    assert np.max(np.abs(z2 - 2 * want)) <= 2e-14 * np.max(np.abs(want)) and np.all(z2[untouched] == 0)
        assert {7: {21, 35, 7}, 16: {11440, 12870, 8008}, 18: {48620, 43758}}[L] == sizes
        # the other kind of factor: a real one on c128; a complex one on an f64 engine is refused
        new = ref.new_sector("splus", ref.UP, L, m)
        want = ref.acc_modified_state_(np.zeros(ref.size(L, new), src.dtype), "splus", L, m, new, src, sites[-1], ref.UP, -1.25)
        if cplx:
            z, _ = e.apply_operator("splus", sites[-1], ref.UP, L, m, 0, src, factor=-1.25, basis="spin_half")
            assert np.max(np.abs(z - want)) <= 1e-14 * np.max(np.abs(want))
        else:
            with pytest.raises(LppError) as ei:
                e.apply_operator("splus", sites[-1], ref.UP, L, m, 0, src, factor=0.75 - 0.5j, basis="spin_half")
            assert ei.value.status == 1
        # refusals are status codes, never a launch
        for op in ("c", "cdagger"):
            with pytest.raises(LppError) as ei:
                e.apply_operator(op, 0, ref.UP, L, m, 0, src, basis="spin_half")
            assert ei.value.status == 1
        with pytest.raises(LppError) as ei:
            e.apply_operator("sminus", 0, ref.UP, L, 0, 0, np.ones(1, src.dtype), basis="spin_half")
        assert ei.value.status == 1
        with pytest.raises(LppError) as ei:
            e.apply_operator("splus", 0, ref.UP, L, L, 0, np.ones(1, src.dtype), basis="spin_half")
        assert ei.value.status == 1
        with pytest.raises(LppError):
            e.apply_operator("sz", L, 0, L, m, 0, src, basis="spin_half")
        with pytest.raises(ValueError):
            e.apply_operator("sz", 0, 0, L, m, 0, src, basis="heisenberg")


def test_apply_operator_heis_long_chain():
    """40 sites, three up spins (9880 states; 780 after S-): the cut of the word is at 14 bits there -- the largest LDS tables, 64 KiB -- and most runs
    hold one element.  The word list of 2^40 words cannot be searched; the expected vector comes from the expanded plan, which
    tests/test_heis_observables_host.py checks against a direct enumeration at 62 sites."""
    L, m = 40, 3
    src = oracle.fill_random(9880, 5)
    with LanczosEngine() as e:
        for op, site in (("sminus", 0), ("sminus", 13), ("sminus", 14), ("sminus", 39), ("sz", 13), ("sz", 39), ("n", 20), ("splus", 5), ("splus", 30)):
            plan = operator_plan_heis(op, site, ref.DOWN, L, m)
            assert plan["lb"] == 14
            a = plan["action"]
            want = np.where(a != 0, np.sign(a) * src[np.maximum(np.abs(a) - 1, 0)], 0.0)
            z, parts = e.apply_operator(op, site, ref.DOWN, L, m, 0, src, basis="spin_half")
            assert parts == (plan["nup"], 0) and len(z) == len(a) and np.any(want != 0)
            assert np.array_equal(z, want), (op, site)


def test_spins_above_one_half_are_refused():
    """twiceS = 2: the reference throws (BasisHeisenberg.h:130, Heisenberg.h:223); two_point and spectral_function answer LPP_ERR_INVALID"""
    with LanczosEngine() as e:
        e.assemble_heisenberg(6, 6, chain(6, 1.0, True), chain(6, 1.0, True), twiceS=2)
        e.keep_states(1)
        e.lanczos(1, want_vectors=False)
        for call in (lambda: e.two_point("sz"), lambda: e.spectral_function("sz", 0, 0), lambda: e.spectral_function("splus", 0, 1)):
            with pytest.raises(LppError) as ei:
                call()
            assert ei.value.status == 1
        assert e.sector_assemblies == 0


# ---- 2. / 3. resident states and two-point correlations ------------------------------------------------------------------------------------------
def _ring16():
    L, m = 16, 8
    return L, m, chain(L, 1.0, True), chain(L, 0.7, True), np.linspace(-0.3, 0.4, L)


def test_resident_states_on_the_chain_form(monkeypatch):
    """keep_states(2) on the forced chain form: state(k) is the host Ritz vector"""
    L, m, jpm, jzz, h = _ring16()
    _force_chain(monkeypatch, True)
    with LanczosEngine(reortho=True, max_steps=150, eps=1e-11) as e:
        e.assemble_heisenberg(L, m, jpm, jzz, h)
        assert e.layout()["kernel"] == 4
        e.keep_states(2)
        eg, zg, _ = e.lanczos(2, want_vectors=True)
        A = oracle.heis_csr(L, 1, m, jpm, jzz, h)
        eo, _, _ = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234), nstates=2, max_steps=150, eps=1e-11, reortho=True, want_vectors=False)
        assert rel(eg, eo) < 1e-8
        for k in (0, 1):
            ptr, n = e.state_device(k)
            assert n == e.rows() == ref.size(L, m) and ptr % 16 == 0
            assert rel(e.state(k), zg[k]) <= 1e-12


@pytest.mark.parametrize("chain_form", [True, False])
def test_two_point_heis(chain_form, monkeypatch):
    """-c sz / n / splus / sminus on the chain form and on the general layout of the same ring, (16;8) with a site-dependent field"""
    L, m, jpm, jzz, h = _ring16()
    _force_chain(monkeypatch, chain_form)
    with LanczosEngine(reortho=True, max_steps=150, eps=1e-11) as e:
        e.assemble_heisenberg(L, m, jpm, jzz, h)
        assert (e.layout()["kernel"] == 4) == chain_form
        e.keep_states(2)
        eg, zg, _ = e.lanczos(2, want_vectors=True)
        gs = e.state(0)
        assert rel(gs, zg[0]) <= 1e-12
        got = {}
        for op, spins in (("sz", (0, 0)), ("n", (0, 0)), ("n", (0, 1)), ("splus", (0, 0)), ("sminus", (0, 0))):
            res, tr = e.two_point(op, spins)
            want, wtr = ref.two_point(op, L, m, gs, gs, spins)
            scale = np.max(np.abs(want))
            print("two_point Heisenberg %s %s chain form %s: max deviation %.3e of %.3e" % (op, spins, chain_form, np.max(np.abs(res - want)), scale))
            assert np.max(np.abs(res - want)) <= 1e-12 * scale, (op, spins)
            assert abs(tr - np.trace(res)) <= 1e-12 * scale and abs(tr - wtr) <= 1e-11 * scale
            got[(op, spins)] = tr
        # sum_i <S^z_i S^z_i> = L/4, sum_i <n_up,i> = szPlusConst, sum_i <S^-_i S^+_i> = the down spins
        assert abs(got[("sz", (0, 0))] - L / 4) <= 1e-10 and abs(got[("n", (0, 0))] - m) <= 1e-10 and abs(got[("splus", (0, 0))] - (L - m)) <= 1e-10
        # <bra| ... |ket> between two resident states
        for op, spins in (("sz", (0, 0)), ("splus", (0, 0)), ("n", (0, 1))):
            res, tr = e.two_point(op, spins, bra=1, ket=0)
            want, wtr = ref.two_point(op, L, m, e.state(1), gs, spins)
            # absolute: the two states are orthogonal, so the entries can be small; each is a dot product of two vectors of norm <= 1 (|A psi| <= |psi|
            # for every operator here) over 12870 terms, whose rounding error is far below 12870 * 1.1e-16 * 1 = 1.4e-12
            assert np.max(np.abs(want)) > 1e-6 and np.max(np.abs(res - want)) <= 1e-12, (op, spins)
            assert abs(tr - wtr) <= 1e-11
        with pytest.raises(LppError):
            e.two_point("splus", (0, 1))  # the reference throws
        with pytest.raises(LppError) as ei:
            e.two_point("c", (0, 0))  # hasNewParts throws
        assert ei.value.status == 1


def test_two_point_and_spectral_with_an_anisotropy():
    """twiceS = 1 with AnisotropyD goes through the any-spin assembler; its basis is the same word list, and so are the observables.  (10;5): 252 states."""
    L, m = 10, 5
    jpm, jzz, h, d = chain(L, 1.0, True), chain(L, 0.8, True), np.linspace(-0.2, 0.3, L), np.linspace(0.1, 0.4, L)
    with LanczosEngine() as e:
        e.assemble_heisenberg(L, m, jpm, jzz, h, twiceS=1, anisotropy=d)
        A = oracle.heis_csr(L, 1, m, jpm, jzz, h, aniso=d)
        rp, ci, va = e.get_csr()
        assert np.array_equal(rp, A.rowptr) and np.array_equal(ci, A.colind) and rel(va, A.values) < 1e-14
        e.keep_states(1)
        eg, zg, _ = e.lanczos(1, want_vectors=True)
        gs = e.state(0)
        assert rel(gs, zg[0]) <= 1e-12
        for op in ("sz", "splus"):
            res, tr = e.two_point(op, (0, 0))
            want, wtr = ref.two_point(op, L, m, gs, gs, (0, 0))
            assert np.max(np.abs(res - want)) <= 1e-12 * np.max(np.abs(want)) and abs(tr - wtr) <= 1e-11 * np.max(np.abs(want))
        recs = e.spectral_function("splus", 1, 4, ref.UP)
        want = ref.spectral_types("splus", L, m, gs, 1, 4, ref.UP)
        assert [r["type"] for r in recs] == [0, 1, 2, 3]
        for r, (typ, o, new, modif, ws2, msign) in zip(recs, want):
            assert r["sector"] == (new, 0) and abs(r["weight"] - ws2) <= 1e-12 * abs(ws2)
            steps, ao, bo, _, _ = oracle.lanczos_decomposition(oracle.heis_csr(L, 1, new, jpm, jzz, h, aniso=d), modif)
            assert r["steps"] == steps and rel(r["a"], ao) < 1e-8 and rel(r["b"], bo) < 1e-8, typ
        assert e.sector_assemblies == 2


# ---- 4. spectral function -----------------------------------------------------------------------------------------------------------------------
_DENSE = {}


def _dense_sector(key, A):
    if key not in _DENSE:
        _DENSE[key] = np.linalg.eigh(A.to_scipy().toarray())
    return _DENSE[key]


def _lehmann(w_eig, v_eig, modif, ws2, sigma, eg, z):
    ov = np.abs(v_eig.conj().T @ modif) ** 2
    wn = np.vdot(modif, modif).real
    return (ws2 / wn) * np.sum(ov[None, :] / (z[:, None] + sigma * (w_eig[None, :] - eg)), axis=1)


def test_spectral_function_heis():
    """-g sz and -g splus on (12;6) of tests/golden/heisenberg_chain_L12.inp: types, sectors, sigma and weights as the restatement, a / b against
    the oracle's decomposition of the restatement's modified vector on the oracle's matrix of the new sector, the Lehmann sum from the dense
    spectrum of that sector (924 and 792 states), and the sum rules of a diagonal pair."""
    L, m, jpm, jzz, field = _golden_model()
    assert (L, m) == (12, 6)
    omega = np.arange(-8.0, 8.0 + 1e-9, 0.25) + 0.1j
    with LanczosEngine() as e:
        e.assemble_heisenberg(L, m, jpm, jzz, field)
        e.keep_states(1)
        eg, zg, _ = e.lanczos(1, want_vectors=True)
        gs = e.state(0)
        before = gs.copy()
        for op in ("sz", "splus"):
            for (i, j) in ((0, 0), (0, 3), (2, 5)):
                recs = e.spectral_function(op, i, j, ref.UP)
                want = ref.spectral_types(op, L, m, gs, i, j, ref.UP)
                assert [r["type"] for r in recs] == [t[0] for t in want] and len(recs) == (2 if i == j else 4)
                for r, (typ, o, new, modif, ws2, msign) in zip(recs, want):
                    assert r["sector"] == (new, 0) and r["sigma"] == msign and r["Eg"] == eg[0]
                    assert new == {"sz": 6, "splus": 7, "sminus": 5}[o]
                    assert abs(r["weight"] - ws2) <= 1e-12 * abs(ws2), (op, i, j, typ, r["weight"], ws2)
                    A = oracle.heis_csr(L, 1, new, jpm, jzz, field)
                    assert A.nrows in (792, 924)
                    steps, ao, bo, _, _ = oracle.lanczos_decomposition(A, modif)
                    assert r["steps"] == steps and rel(r["a"], ao) < 1e-8 and rel(r["b"], bo) < 1e-8, (op, i, j, typ)
                    w_eig, v_eig = _dense_sector(new, A)
                    exact = _lehmann(w_eig, v_eig, modif, ws2, msign, eg[0], omega)
                    g_gpu = continued_fraction(r, omega)
                    g_orc = continued_fraction(dict(a=ao, b=bo, Eg=eg[0], weight=ws2, sigma=msign), omega)
                    scale = np.max(np.abs(exact))
                    d_orc, d_gpu = np.max(np.abs(g_orc - exact)) / scale, np.max(np.abs(g_gpu - exact)) / scale
                    print("lehmann Heisenberg %s pair (%d,%d) type %d: oracle %.3e gpu %.3e" % (op, i, j, typ, d_orc, d_gpu))
                    # ten times what the oracle's own decomposition of the same vector deviates from the Lehmann sum by (tests/test_gpu_tj_observables.py)
                    assert d_gpu <= 10 * d_orc, (op, i, j, typ, d_gpu, d_orc)
                if i == j:
                    w = {r["type"]: r["weight"] for r in recs}
                    if op == "sz":  # the raw sz is -2 S^z and the state is accumulated twice: |2 (-2 S^z) gs|^2 = 4, s2 = +1 / -1
                        assert abs(w[0] - 4.0) <= 1e-10 and abs(w[1] + 4.0) <= 1e-10
                    else:  # 4 <S+ S-> + 4 <S- S+> = 4
                        assert w[0] > 0 > w[1] and abs(w[0] - w[1] - 4.0) <= 1e-10
        assert e.sector_assemblies == 3 and sorted(e._sectors) == [(5, 0), (6, 0), (7, 0)]  # the engine's own sector has an engine of its own
        assert np.array_equal(e.state(0).view(np.uint64), before.view(np.uint64))
        with pytest.raises(LppError) as ei:
            e.spectral_function("c", 0, 0)
        assert ei.value.status == 1 and e.sector_assemblies == 3


# ---- 5. the C ABI: a decomposition on the engine that holds the state ---------------------------------------------------------------------------
def test_spectral_decomposition_heis_on_the_engine_itself():
    """lpp_engine_spectral_decomposition_heis with sector == e (sz stays in the sector): the resident state is unchanged bit for bit"""
    L, m, jpm, jzz, field = _golden_model()
    with LanczosEngine() as e:
        e.assemble_heisenberg(L, m, jpm, jzz, field)
        e.keep_states(1)
        e.lanczos(1, want_vectors=False)
        before = e.state(0)
        a, b = np.zeros(e.max_steps + 2), np.zeros(e.max_steps + 2)
        n, w, st = C.c_int32(), C.c_double(), Stats()
        status = e._lib.lpp_engine_spectral_decomposition_heis(e._h, 0, e._h, 2, 0, 3, 0, 1.0, L, m, 0, C.byref(w), C.byref(n), a.ctypes.data_as(C.c_void_p),
                                                               b.ctypes.data_as(C.c_void_p), C.byref(st))
        assert status == 0
        modif = ref.modified_state("sz", L, m, m, before, 1, 0, 3, ref.UP)
        assert abs(w.value - np.vdot(modif, modif)) <= 1e-12 * w.value
        steps, ao, bo, _, _ = oracle.lanczos_decomposition(oracle.heis_csr(L, 1, m, jpm, jzz, field), modif)
        assert n.value == steps and rel(a[:steps], ao) < 1e-8 and rel(b[:steps], bo) < 1e-8
        assert np.array_equal(e.state(0).view(np.uint64), before.view(np.uint64))
        # a sector engine of another size is refused
        status = e._lib.lpp_engine_spectral_decomposition_heis(e._h, 0, e._h, 5, 0, 3, 0, 1.0, L, m, 0, C.byref(w), C.byref(n), a.ctypes.data_as(C.c_void_p),
                                                               b.ctypes.data_as(C.c_void_p), C.byref(st))
        assert status == 1


# ---- 6. the lanczos driver: -c, -g on a Heisenberg input -----------------------------------------------------------------------------------------
def _python_engine():
    """the Python path on the model of the input file, started from the vector the C++ shim starts from (fillRandom, seed 1234)"""
    L, m, jpm, jzz, field = _golden_model()
    e = LanczosEngine()
    e.assemble_heisenberg(L, m, jpm, jzz, field)
    e.keep_states(1)
    e.lanczos(1, init=oracle.fill_random(e.rows(), 1234), want_vectors=False)
    return e, L


@pytest.mark.parametrize("op,trace", [("sz", 3.0), ("splus", 6.0)])
def test_driver_two_point_heis(op, trace):
    """lanczos -f tests/golden/heisenberg_chain_L12.inp -c <op>: the matrix and the MatrixDiagonal line against two_point of the Python path"""
    assert os.path.exists(DRIVER), "run __graft_entry__.build()"
    res = subprocess.run([DRIVER, "-f", os.path.join(GOLD, NAME), "-c", op, "-p", "14"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    k = next(i for i, ln in enumerate(lines) if ln.startswith("MatrixDiagonal = "))
    assert lines[k - 2] == "spins=0 0" and lines[k - 1] == "orbs=0 0"
    diag = float(lines[k].split("=", 1)[1].strip())
    e, L = _python_engine()
    with e:
        want, wtr = e.two_point(op, (0, 0))
    assert lines[k + 1].split() == [str(L), str(L)]
    got = np.array([[float(x) for x in lines[k + 2 + i].split()] for i in range(L)])
    assert got.shape == (L, L)
    scale = np.max(np.abs(want))
    print("driver Heisenberg -c %s: max deviation %.3e of %.3e, MatrixDiagonal %s against %s" % (op, np.max(np.abs(got - want)), scale, diag, wtr))
    assert np.max(np.abs(got - want)) <= 1e-8 * scale
    assert abs(diag - wtr) <= 1e-8 and abs(diag - trace) <= 1e-8  # L/4, the down spins


def _parse_comb(text):
    """the record layout of INTEGRATION.md"""
    head = dict(re.findall(r"^(Site0|Site1|TSPCenter)=(\d+)$", text, re.M))
    labels = re.search(r"^#INDEXTOCF (.*)$", text, re.M).group(1).split()
    count = int(re.search(r"^#ContinuedFractionCollection=(\d+)$", text, re.M).group(1))
    recs = []
    for block in re.split(r"^#ContinuedFraction=\d+\n", text, flags=re.M)[1:]:
        vec = {}
        for key in ("Avector", "Bvector"):
            toks = re.search(r"^#%s (.*)$" % key, block, re.M).group(1).split()
            assert int(toks[0]) == len(toks) - 1
            vec[key] = np.array([float(x) for x in toks[1:]])
        sc = {k: float(v) for k, v in re.findall(r"^#CF(Energy|Weight|Isign)=(\S+)$", block, re.M)}
        recs.append(dict(a=vec["Avector"], b=vec["Bvector"], Eg=sc["Energy"], weight=sc["Weight"], sigma=sc["Isign"]))
    assert count == len(recs) == len(labels)
    return head, labels, recs


@pytest.mark.parametrize("op,assemblies,sectors", [("sz", 1, {(6, 0)}), ("splus", 2, {(5, 0), (7, 0)})])
def test_driver_spectral_function_heis(op, assemblies, sectors, tmp_path):
    """lanczos -g <op> with `TSPSites 2 0 3` and SpectralSteps=40 appended to a copy of the input writes <input basename>0.comb; its records against
    spectral_function"""
    assert os.path.exists(DRIVER), "run __graft_entry__.build()"
    inp = tmp_path / "heis.inp"
    inp.write_text(open(os.path.join(GOLD, NAME)).read().rstrip("\n") + "\nTSPSites 2 0 3\nSpectralSteps=40\n")
    res = subprocess.run([DRIVER, "-f", str(inp), "-g", op, "-p", "14"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr
    assert "#gf(i=0, j=3)" in res.stdout.splitlines()
    assert "#SectorAssemblies=%d" % assemblies in res.stderr
    comb = tmp_path / "heis.inp0.comb"
    assert comb.exists(), os.listdir(str(tmp_path))
    head, labels, recs = _parse_comb(comb.read_text())
    assert head == {"Site0": "0", "Site1": "3"} and labels == ["0,0,0,0", "0,1,0,0", "0,2,0,0", "0,3,0,0"]
    e, L = _python_engine()
    with e:
        want = e.spectral_function(op, 0, 3, 0, max_steps=40)
        assert [w["label"] for w in want] == labels and {w["sector"] for w in want} == sectors
        for r, w in zip(recs, want):
            print("driver Heisenberg -g %s type %d: steps %d / %d" % (op, w["type"], len(r["a"]), w["steps"]))
            assert len(r["a"]) == len(r["b"]) == w["steps"] <= 40
            assert rel(r["a"], w["a"]) < 1e-8 and rel(r["b"], w["b"]) < 1e-8
            assert abs(r["weight"] - w["weight"]) <= 1e-8 * abs(w["weight"]) and r["sigma"] == w["sigma"]
            assert abs(r["Eg"] - w["Eg"]) <= 1e-8 * abs(w["Eg"])
            z = np.array([-1.0 + 0.1j, 0.5 + 0.1j, 2.0 + 0.1j])
            assert np.max(np.abs(continued_fraction(r, z) - continued_fraction(w, z))) <= 1e-8 * np.max(np.abs(continued_fraction(w, z)))
