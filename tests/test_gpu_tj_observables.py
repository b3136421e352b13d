"""t-J observables on the GPU: operator application in the BasisTjMultiOrbLanczos order, resident states of a hole-major engine, two-point correlations
and spectral functions, against the literal restatement of the reference in tests/tj_obs_reference.py (word list + search, no factorisation).
Tolerances are those of tests/test_gpu_observables.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
import tj_obs_reference as ref
from helpers import chain, rel
from lanczosplusplus_amd import LanczosEngine, LppError, continued_fraction, geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "lanczosplusplus_amd", "host", "lanczos")
GOLD = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu


def _ring(L):
    return chain(L, -1.0, True)


def _tj_ring(L, cplx=False):
    """(hop, jpm, jzz, w) of the t-J ring the existing hole-major tests use; cplx: Peierls phases as tests/test_gpu_observables.py builds them"""
    hop = _ring(L)
    j = 0.5 * np.abs(hop)
    if cplx:
        hop = hop.astype(complex) * np.where(np.triu(np.ones((L, L)), 1) > 0, np.exp(0.37j), np.exp(-0.37j))
    return hop, j, j, np.zeros((L, L))


def _golden_model(name):
    inp = geometry.parse_input(open(os.path.join(GOLD, name)).read())
    assert inp["Model"] == "TjMultiOrb"
    L, nup, ndown = int(inp["TotalNumberOfSites"]), int(inp["TargetElectronsUp"]), int(inp["TargetElectronsDown"])
    return L, (nup, ndown), tuple(geometry.terms_from_input(inp)[:4]), inp.get("potentialV")


# ---- 1. operator application ------------------------------------------------------------------------------------------------------------------
# (7;2,1): 105 states, odd -- the f64 half-unit tail; its c DOWN destination (2,0) has 21.  (8;3,3): 560.  (12;4,4): 34650 and 27720 in (3,4): several
# tiles of 1024 units, and 56 / 70 patterns per down word do not divide a tile, so tiles straddle down words.
@pytest.mark.parametrize("dtype", ["f64", "c128"])
@pytest.mark.parametrize("L,parts", [(7, (2, 1)), (8, (3, 3)), (12, (4, 4))])
def test_apply_operator_tj(dtype, L, parts):
    """every operator and spin (UP only for splus / sminus), sites 0, 3, L-1: each output element is one product"""
    cplx = dtype == "c128"
    n = ref.size(L, *parts)
    assert n == {7: 105, 8: 560, 12: 34650}[L]
    src = oracle.fill_random(n, 11, cplx)
    factor = (0.75 - 0.5j) if cplx else -1.25
    sizes = set()
    with LanczosEngine(dtype=dtype) as e:
        for op in ref.OPS:
            for spin in ((ref.UP,) if op in ("splus", "sminus") else (ref.UP, ref.DOWN)):
                new = ref.new_sector(op, spin, L, *parts)
                for site in (0, 3, L - 1):
                    z, got_parts = e.apply_operator(op, site, spin, L, parts[0], parts[1], src, factor=factor, basis="tj")
                    assert got_parts == new and len(z) == ref.size(L, *new)
                    sizes.add(len(z))
                    want = ref.acc_modified_state_(np.zeros(len(z), src.dtype), op, L, parts, new, src, site, spin, factor)
                    assert np.max(np.abs(want)) > 0
                    assert np.max(np.abs(z - want)) <= 1e-14 * np.max(np.abs(want)), (op, spin, site)
                    idx, _ = ref.action(op, L, parts, new, site, spin)
                    untouched = np.ones(len(z), bool)
                    untouched[idx[idx >= 0]] = False
                    assert untouched.any() and np.all(z[untouched] == 0), (op, spin, site)
                    # z += ...: a second application on top of the first
                    z2, _ = e.apply_operator(op, site, spin, L, parts[0], parts[1], src, factor=factor, out=z, basis="tj")
                    assert np.max(np.abs(z2 - 2 * want)) <= 2e-14 * np.max(np.abs(want)) and np.all(z2[untouched] == 0)
        assert {7: 21, 8: 560, 12: 27720}[L] in sizes
        # refusals are status codes / None, never a launch
        assert e.apply_operator("cdagger", 0, ref.UP, 8, 4, 4, oracle.fill_random(ref.size(8, 4, 4), 1, cplx), basis="tj") == (None, None)
        with pytest.raises(LppError) as ei:
            e.apply_operator("splus", 0, ref.DOWN, L, parts[0], parts[1], src, basis="tj")
        assert ei.value.status == 1
        with pytest.raises(LppError):
            e.apply_operator("c", L, 0, L, parts[0], parts[1], src, basis="tj")
        with pytest.raises(ValueError):
            e.apply_operator("c", 0, 0, L, parts[0], parts[1], src, basis="heisenberg")


# ---- 2. resident state on a hole-major engine ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("save_vectors", [1, 0])
def test_resident_state_on_hole_major_engine(save_vectors, monkeypatch):
    """after keep_states_tj the resident state is the host Ritz vector bit for bit on both Ritz paths (both are permutations of one device vector);
    keep_states keeps its ABI-6 refusal on the same engine"""
    L, parts = 12, (5, 4)
    monkeypatch.setenv("LPP_TJ_LAYOUT", "1")  # below the size from which the form is chosen by itself
    with LanczosEngine(save_vectors=save_vectors) as e:
        e.assemble_tj(L, parts[0], parts[1], *_tj_ring(L))
        assert e.layout()["kernel"] == 5
        with pytest.raises(LppError) as ei:
            e.keep_states(1)
        assert ei.value.status == 5
        e.keep_states_tj(1)
        eg, zg, st = e.lanczos(1, want_vectors=True)
        assert st["vectors_saved"] == save_vectors
        ptr, n = e.state_device(0)
        assert n == e.rows() == ref.size(L, *parts) and ptr % 16 == 0
        assert np.array_equal(e.state(0).view(np.uint64), zg[0].view(np.uint64))
        A = oracle.tj_csr(L, parts[0], parts[1], *_tj_ring(L))
        eo, _, _ = oracle.lanczos_solve(A, oracle.fill_random(A.nrows, 1234), want_vectors=False)
        assert abs(eg[0] - eo[0]) <= 1e-10 * abs(eo[0])
        # the ABI-6 calls answer a hole-major engine as before: its keep, and a device start vector
        with pytest.raises(LppError) as ei:
            e.decomposition(init_device=ptr)
        assert ei.value.status == 5
        with pytest.raises(LppError) as ei:
            e.keep_states(1)
        assert ei.value.status == 5
        e.keep_states(0)  # ... which withdraws the permission again: nothing is kept, the solve runs
        e.lanczos(1, want_vectors=False)
        with pytest.raises(LppError):
            e.state_device(0)


# ---- 3. two-point correlations ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["1", "0"])
def test_two_point_tj(layout, monkeypatch):
    """on the hole-major engine and on the general layout of the same model"""
    L, (nup, ndown) = 12, (5, 4)
    monkeypatch.setenv("LPP_TJ_LAYOUT", layout)
    with LanczosEngine() as e:
        e.assemble_tj(L, nup, ndown, *_tj_ring(L))
        assert (e.layout()["kernel"] == 5) == (layout == "1")
        e.keep_states_tj(1)
        eg, zg, _ = e.lanczos(1, want_vectors=True)
        gs = zg[0]
        got = {}
        for op, spins in (("c", (0, 0)), ("c", (1, 1)), ("n", (0, 0)), ("sz", (0, 0)), ("splus", (0, 0))):
            res, tr = e.two_point(op, spins)
            want, wtr = ref.two_point(op, L, (nup, ndown), gs, gs, spins)
            scale = np.max(np.abs(want))
            print("two_point t-J %s %s layout %s: max deviation %.3e of %.3e" % (op, spins, layout, np.max(np.abs(res - want)), scale))
            assert np.max(np.abs(res - want)) <= 1e-12 * scale, (op, spins)
            assert abs(tr - np.trace(res)) <= 1e-12 * scale and abs(tr - wtr) <= 1e-11 * scale
            got[(op, spins)] = (res, tr)
        assert abs(got[("c", (0, 0))][1] - nup) <= 1e-10 and abs(got[("c", (1, 1))][1] - ndown) <= 1e-10
        assert np.max(np.abs(np.diag(got[("n", (0, 0))][0]) - np.diag(got[("c", (0, 0))][0]))) <= 1e-10
        with pytest.raises(LppError):
            e.two_point("c", (0, 1))  # the reference throws
        with pytest.raises(LppError) as ei:
            e.two_point("splus", (1, 1))  # the reference ranks words outside the basis
        assert ei.value.status == 1
        with pytest.raises(LppError) as ei:
            e.reduced_density_matrix(4)  # not for this basis, as before
        assert ei.value.status == 5


def test_two_point_tj_no_sector_keeps_the_fill():
    """cdagger without holes, (8;4,4): the sector does not exist, the matrix keeps the -100 fill"""
    L = 8
    with LanczosEngine() as e:
        e.assemble_tj(L, 4, 4, *_tj_ring(L))
        e.keep_states_tj(1)
        e.lanczos(1, want_vectors=False)
        for spins in ((0, 0), (1, 1)):
            res, tr = e.two_point("cdagger", spins)
            assert np.all(res == -100.0) and tr == 0
        res, tr = e.two_point("c", (0, 0))
        assert abs(tr - 4) <= 1e-10


def test_two_point_tj_between_two_complex_states():
    """c128, two resident states, bra != ket: the bra side (the left factor) is the conjugated one.  (8;3,3) ring with Peierls phases."""
    L, parts = 8, (3, 3)
    with LanczosEngine(dtype="c128") as e:
        e.assemble_tj(L, parts[0], parts[1], *_tj_ring(L, cplx=True))
        e.keep_states_tj(2)
        _, zg, _ = e.lanczos(2, want_vectors=True)
        for k in (0, 1):
            assert np.array_equal(e.state(k).view(np.uint64), zg[k].view(np.uint64))
        for op, spins, bra, ket in (("c", (0, 0), 1, 0), ("c", (1, 1), 0, 1), ("n", (0, 1), 1, 0), ("sz", (0, 1), 1, 0), ("sminus", (0, 0), 1, 0)):
            res, tr = e.two_point(op, spins, bra=bra, ket=ket)
            want, wtr = ref.two_point(op, L, parts, zg[bra], zg[ket], spins)
            scale = np.max(np.abs(want))
            print("two_point t-J %s %s <%d|..|%d>: max deviation %.3e of %.3e" % (op, spins, bra, ket, np.max(np.abs(res - want)), scale))
            assert np.max(np.abs(res - want)) <= 1e-12 * scale, (op, spins, bra, ket)  # sums of at most 560 products of normalised vectors
            assert abs(tr - wtr) <= 1e-11 * scale
        r10, _ = e.two_point("c", (0, 0), bra=1, ket=0)
        r01, _ = e.two_point("c", (0, 0), bra=0, ket=1)
        assert np.max(np.abs(r10 - r01.conj().T)) <= 1e-12 * np.max(np.abs(r10))


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


def test_spectral_function_tj():
    """-g c, both spins, on (8;3,3) of tests/golden/tj_chain_L8_complex.inp (its potentialV lifts the ground state's degeneracy): types, sectors and
    weights as the restatement, a / b against the oracle's decomposition of the restatement's modified vector on the oracle's matrix of the new
    sector, the Lehmann sum from the dense spectrum of that sector, and the sum rule of a diagonal pair."""
    L, parts, terms, pv = _golden_model("tj_chain_L8_complex.inp")
    assert (L, parts) == (8, (3, 3))
    omega = np.arange(-8.0, 8.0 + 1e-9, 0.25) + 0.1j
    with LanczosEngine(dtype="c128") as e:
        e.assemble_tj(L, parts[0], parts[1], *terms, potentialV=pv)
        e.keep_states_tj(1)
        eg, zg, _ = e.lanczos(1, want_vectors=True)
        gs = zg[0]
        nocc = {s: np.diag(e.two_point("n", (s, s))[0]).real for s in (ref.UP, ref.DOWN)}
        for spin in (ref.UP, ref.DOWN):
            for (i, j) in ((0, 0), (0, 3), (2, 5)):
                recs = e.spectral_function("c", i, j, spin)
                want = ref.spectral_types("c", L, parts, gs, i, j, spin)
                assert [r["type"] for r in recs] == [t[0] for t in want] and len(recs) == (2 if i == j else 4)
                for r, (typ, o, new, modif, ws2, msign) in zip(recs, want):
                    assert r["sector"] == new and r["sigma"] == msign and r["Eg"] == eg[0]
                    assert abs(r["weight"] - ws2) <= 1e-12 * abs(ws2), (spin, i, j, typ, r["weight"], ws2)
                    A = oracle.tj_csr(L, new[0], new[1], *terms, potentialV=pv, force_complex=True)
                    assert A.nrows <= 560
                    steps, ao, bo, _, _ = oracle.lanczos_decomposition(A, modif)
                    assert r["steps"] == steps and rel(r["a"], ao) < 1e-8 and rel(r["b"], bo) < 1e-8, (spin, i, j, typ)
                    w_eig, v_eig = _dense_sector(new, A)
                    exact = _lehmann(w_eig, v_eig, modif, ws2, msign, eg[0], omega)
                    g_gpu = continued_fraction(r, omega)
                    g_orc = continued_fraction(dict(a=ao, b=bo, Eg=eg[0], weight=ws2, sigma=msign), omega)
                    scale = np.max(np.abs(exact))
                    d_orc, d_gpu = np.max(np.abs(g_orc - exact)) / scale, np.max(np.abs(g_gpu - exact)) / scale
                    print("lehmann t-J spin %d pair (%d,%d) type %d: oracle %.3e gpu %.3e" % (spin, i, j, typ, d_orc, d_gpu))
                    # ten times what the oracle's own decomposition of the same vector deviates from the Lehmann sum by: the decomposition stops
                    # when the lowest Ritz value has converged, so the truncated fraction is off the full sum by the same amount for both
                    assert d_gpu <= 10 * d_orc, (spin, i, j, typ, d_gpu, d_orc)
                if i == j:
                    # c_{i s} c+_{i s} + c+_{i s} c_{i s} = 1 - n_{i,-s} without double occupancy; the state is accumulated twice: a factor 4
                    w = sum(r["weight"] for r in recs)
                    assert abs(w - 4.0 * (1.0 - nocc[1 - spin][i])) <= 1e-10, (spin, i, w)
        assert e.sector_assemblies == 4  # (2,3), (4,3), (3,2), (3,4): kept, keyed by sector
        for op in ("n", "sz"):
            with pytest.raises(LppError):
                e.spectral_function(op, 0, 0)
        with pytest.raises(LppError) as ei:
            e.spectral_function("splus", 0, 0, ref.DOWN)
        assert ei.value.status == 1 and e.sector_assemblies == 4


def test_spectral_function_tj_hole_major(monkeypatch):
    """the same operator on the hole-major pair (12;5,4) -> (4,4) and (6,4): the sector engines are hole-major too (126, 70 and 210 patterns per
    hole configuration, all >= 64) and start from the device vector through their permutation"""
    L, parts = 12, (5, 4)
    model = _tj_ring(L)
    monkeypatch.setenv("LPP_TJ_LAYOUT", "1")
    with LanczosEngine() as e:
        e.assemble_tj(L, parts[0], parts[1], *model)
        assert e.layout()["kernel"] == 5
        e.keep_states_tj(1)
        eg, zg, _ = e.lanczos(1, want_vectors=True)
        gs = zg[0]
        for (i, j) in ((0, 0), (2, 5)):
            recs = e.spectral_function("c", i, j, ref.UP)
            want = ref.spectral_types("c", L, parts, gs, i, j, ref.UP)
            assert [r["type"] for r in recs] == [t[0] for t in want] and len(recs) == (2 if i == j else 4)
            for r, (typ, o, new, modif, ws2, msign) in zip(recs, want):
                assert r["sector"] == new and new in ((4, 4), (6, 4))
                assert abs(r["weight"] - ws2) <= 1e-12 * abs(ws2)
                A = oracle.tj_csr(L, new[0], new[1], *model)
                steps, ao, bo, _, _ = oracle.lanczos_decomposition(A, modif)
                print("hole-major -g c pair (%d,%d) type %d: steps %d / %d a %.3e b %.3e" % (i, j, typ, r["steps"], steps, rel(r["a"], ao) if r["steps"] == steps else -1,
                                                                                         rel(r["b"], bo) if r["steps"] == steps else -1))
                assert r["steps"] == steps and rel(r["a"], ao) < 1e-8 and rel(r["b"], bo) < 1e-8, (i, j, typ)
        assert e.sector_assemblies == 2 and sorted(e._sectors) == [(4, 4), (6, 4)]
        for eng in e._sectors.values():
            assert eng.layout()["kernel"] == 5


# ---- 5. the lanczos driver: -c, -g on t-J inputs -----------------------------------------------------------------------------------------------
def _python_engine_of(name):
    """the Python path on the model of an input file, started from the vector the C++ shim starts from (fillRandom, seed 1234)"""
    L, parts, terms, pv = _golden_model(name)
    e = LanczosEngine(dtype="c128")  # SolverOptions=useComplex
    e.assemble_tj(L, parts[0], parts[1], *terms, potentialV=pv)
    e.keep_states_tj(1)
    e.lanczos(1, init=oracle.fill_random(e.rows(), 1234, True), want_vectors=False)
    return e, L


def _cplx(tok):
    m = re.match(r"^\(([^,]+),([^)]+)\)$", tok)
    return complex(float(m.group(1)), float(m.group(2))) if m else complex(float(tok))


def test_driver_two_point_tj():
    """lanczos -f tests/golden/tj_chain_L8_complex.inp -c c: the matrix and the MatrixDiagonal line against two_point of the Python path"""
    assert os.path.exists(DRIVER), "run __graft_entry__.build()"
    name = "tj_chain_L8_complex.inp"
    res = subprocess.run([DRIVER, "-f", os.path.join(GOLD, name), "-c", "c", "-p", "14"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    k = next(i for i, ln in enumerate(lines) if ln.startswith("MatrixDiagonal = "))
    assert lines[k - 2] == "spins=0 0" and lines[k - 1] == "orbs=0 0"
    diag = _cplx(lines[k].split("=", 1)[1].strip())
    e, L = _python_engine_of(name)
    with e:
        want, wtr = e.two_point("c", (0, 0))
    assert lines[k + 1].split() == [str(L), str(L)]
    got = np.array([[_cplx(x) for x in lines[k + 2 + i].split()] for i in range(L)])
    assert got.shape == (L, L)
    scale = np.max(np.abs(want))
    print("driver t-J -c c: max deviation %.3e of %.3e, MatrixDiagonal %s against %s" % (np.max(np.abs(got - want)), scale, diag, wtr))
    assert np.max(np.abs(got - want)) <= 1e-8 * scale
    assert abs(diag - wtr) <= 1e-8 and abs(diag - 3) <= 1e-8  # N_up


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


@pytest.mark.parametrize("name,layout,sectors", [("tj_chain_L8_complex.inp", None, {(4, 3), (2, 3)}), ("tj_chain_L12_complex.inp", "1", {(6, 5), (4, 5)})])
def test_driver_spectral_function_tj(name, layout, sectors, tmp_path, monkeypatch):
    """lanczos -g c with `TSPSites 2 0 0` and SpectralSteps=40 appended to a copy of the input writes <input basename>0.comb; its records against
    spectral_function.  The 12-site input with LPP_TJ_LAYOUT=1: (5,5) and both of its sector engines are hole-major."""
    assert os.path.exists(DRIVER), "run __graft_entry__.build()"
    env = dict(os.environ, LPP_VERBOSE="1")
    if layout is not None:
        env["LPP_TJ_LAYOUT"] = layout
        monkeypatch.setenv("LPP_TJ_LAYOUT", layout)
    inp = tmp_path / "tj.inp"
    inp.write_text(open(os.path.join(GOLD, name)).read().rstrip("\n") + "\nTSPSites 2 0 0\nSpectralSteps=40\n")
    res = subprocess.run([DRIVER, "-f", str(inp), "-g", "c", "-p", "14"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path), env=env)
    assert res.returncode == 0, res.stderr
    assert "#gf(i=0, j=0)" in res.stdout.splitlines()
    assert "#SectorAssemblies=2" in res.stderr
    if layout == "1":
        assert len(re.findall(r"t-J hole-major form: \d+ hole configurations", res.stderr)) == 3, res.stderr[-3000:]
    comb = tmp_path / "tj.inp0.comb"
    assert comb.exists(), os.listdir(str(tmp_path))
    head, labels, recs = _parse_comb(comb.read_text())
    assert head == {"Site0": "0", "Site1": "0"} and labels == ["0,0,0,0", "0,1,0,0"]
    e, L = _python_engine_of(name)
    with e:
        assert (e.layout()["kernel"] == 5) == (layout == "1")
        want = e.spectral_function("c", 0, 0, 0, max_steps=40)
        assert [w["label"] for w in want] == labels and {w["sector"] for w in want} == sectors
        if layout == "1":
            assert all(eng.layout()["kernel"] == 5 for eng in e._sectors.values())
        for r, w in zip(recs, want):
            print("driver t-J -g c %s type %d: steps %d / %d" % (name, w["type"], len(r["a"]), w["steps"]))
            assert len(r["a"]) == len(r["b"]) == w["steps"] <= 40  # (the 8-site sectors converge before SpectralSteps)
            assert rel(r["a"], w["a"]) < 1e-8 and rel(r["b"], w["b"]) < 1e-8
            assert abs(r["weight"] - w["weight"]) <= 1e-8 * abs(w["weight"]) and r["sigma"] == w["sigma"]
            assert abs(r["Eg"] - w["Eg"]) <= 1e-8 * abs(w["Eg"])
            z = np.array([-1.0 + 0.1j, 0.5 + 0.1j, 2.0 + 0.1j])
            assert np.max(np.abs(continued_fraction(r, z) - continued_fraction(w, z))) <= 1e-8 * np.max(np.abs(continued_fraction(w, z)))
